"""GPU: the logits coder (``ns_encode_step`` / ``ns_decode_step`` / ``ns_sample_step``; one-wave form, split form and
wide path) against the CPU oracle across vocabulary sizes and row strides.

Bar: bit-exact tokens, decoded bits and per-step (k, k', sel, n, token) traces -- the oracle runs are those of
``tests/coder_vocab_cases.py``, which ``tests/test_coder_vocab_host.py`` checks on the CPU.  The oracle sees
``row[:V]`` only.  The kernel sees rows whose pad columns ``[V, ld)`` are POISONED (stream 0: NaN, stream 1: +inf,
stream 2: the dtype's largest finite value), so a read of a pad column as an id shows up as a range error, a token
``>= V`` or a different trace.  Every case runs twice: with ``ld = row_stride(V)`` on a matrix of its own, and as a
view ``[B, row_stride(V) + 192]`` into a wider poisoned buffer (non-zero, 16-byte aligned offset; the rows' stride is
larger than the view's width).  Both must give the oracle's tokens.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from neuralsteganography_amd import synthetic
from oracle import oracle
from tests import coder_vocab_cases as cv
from tests.coder_vocab_cases import B, CASES, geometry

pytestmark = pytest.mark.gpu

LAYOUTS = ("tight", "view")
VIEW_EXTRA, VIEW_OFFSET, VIEW_BEYOND = 192, 8, 64  # elements: wider view, its offset in the buffer, columns after it


def _torch():
    import torch

    return torch


@pytest.fixture(autouse=True, params=["wave", "split"])
def coder_form(request):
    """Every test runs with both single-pass coder forms: one wave per stream, and the split form (one workgroup
    per stream) forced at every batch size (it applies where the stratified sample is on)."""
    from neuralsteganography_amd import _lib

    prev = _lib.set_split_max_batch(0 if request.param == "wave" else 1 << 30)
    yield request.param
    _lib.set_split_max_batch(prev)


def _poison(s, npdt):
    return (np.nan, np.inf, float(np.finfo(npdt).max))[s % 3]


def _host_rows(row_fn, nstreams, nsteps):
    """[nsteps, nstreams, V]: row_fn(s, t) of every stream and step, in the rows' own dtype."""
    first = row_fn(0, 0)
    out = np.empty((nsteps, nstreams, first.size), first.dtype)
    for t in range(nsteps):
        for s in range(nstreams):
            out[t, s] = row_fn(s, t)
    return out


def _device_rows(rows, dtype, layout):
    """``fn(t)`` -> the ``[nstreams, ld]`` device matrix of step t.  Everything but ``[:, :V]`` holds the stream's
    poison.  'tight': ``ld = row_stride(V)``, a matrix of its own.  'view': ``ld = row_stride(V) + 192`` columns
    starting at column 8 of rows 64 columns wider (one spare poisoned row at the end, so the row range the kernel's
    buffer descriptor covers, ``stride(0)`` elements from each row's start, lies inside the allocation)."""
    from neuralsteganography_amd.coder import row_stride

    torch = _torch()
    nsteps, n, V = rows.shape
    rs = row_stride(V, dtype)
    if layout == "tight":
        ld, off, width, nrow = rs, 0, rs, n
    else:
        ld, off, width, nrow = rs + VIEW_EXTRA, VIEW_OFFSET, rs + VIEW_EXTRA + VIEW_BEYOND, n + 1
    host = np.empty((nsteps, nrow, width), rows.dtype)
    for s in range(nrow):
        host[:, s, :] = _poison(min(s, n - 1), rows.dtype)
    host[:, :n, off:off + V] = rows
    dev = torch.from_numpy(host).cuda()

    def fn(t, _last=None):
        m = dev[t, :n, off:off + ld]
        assert m.shape == (n, ld) and m.stride() == (width, 1) and m.data_ptr() % 16 == 0
        return m

    return fn


def _run_against_oracle(ctx, rows, dtype, expect, *, quality=None, alternate_exact=False):
    """Encode ``expect``'s payloads on ``rows`` in both layouts, step by step against the oracle's traces; then
    decode the tokens back.  ``alternate_exact``: force the exact row sum on odd steps (wide path)."""
    from neuralsteganography_amd.coder import DecodeSession, EncodeSession

    n = len(expect)
    nmax = max(len(e.tokens) for e in expect)
    V = rows.shape[2]
    for layout in LAYOUTS:
        fn = _device_rows(rows, dtype, layout)
        sess = EncodeSession(ctx, [e.bits for e in expect], max_tokens=nmax + 8, quality=quality)
        sess.enable_trace()
        for t in range(nmax):
            sess.step(fn(t), force_exact=alternate_exact and t % 2 == 1)
            tr = sess.trace_rows()
            for s in range(n):
                if t < len(expect[s].traces):
                    got = (int(tr.k[s]), int(tr.kprime[s]), int(tr.sel[s]), int(tr.n[s]), int(tr.token[s]))
                    assert got == expect[s].traces[t], \
                        f"{layout} stream {s} step {t}: kernel {got} oracle {expect[s].traces[t]}"
        toks = sess.tokens()  # raises the streams' range errors
        assert sess.all_done()
        assert all(0 <= tok < V for tl in toks for tok in tl), f"{layout}: a token outside the vocabulary"
        assert toks == [e.tokens for e in expect], f"{layout}: tokens differ from the oracle"
        dec = DecodeSession(ctx, toks, quality=quality)
        for t in range(dec.T):
            dec.step(fn(t), force_exact=alternate_exact and t % 2 == 1)
        out = dec.bits()
        for s in range(n):
            assert out[s] == expect[s].decoded, f"{layout} stream {s}: decoded bits differ from the oracle"
            assert out[s][: len(expect[s].bits)] == expect[s].bits, f"{layout} stream {s}: payload not recovered"


def _params(case, banned=None):
    from neuralsteganography_amd.coder import CoderParams

    return CoderParams(vocab=case.vocab, precision=case.precision, temp=case.temp, topk=case.topk, dtype=case.dtype,
                       banned=banned)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_coder_matches_oracle(case):
    from neuralsteganography_amd.coder import CoderContext

    expect = cv.expected(case)
    ctx = CoderContext(_params(case), max_batch=B)
    assert ctx.wide == cv.is_wide(case.vocab, case.dtype, case.topk)
    rows = _host_rows(lambda s, t: cv.case_row(case, s, t), B, max(len(e.tokens) for e in expect))
    _run_against_oracle(ctx, rows, case.dtype, expect, alternate_exact=ctx.wide)


@pytest.mark.parametrize("vocab,dtype,precision,topk", cv.UNSUPPORTED_WIDE)
def test_wide_context_beyond_17_bit_ids_is_refused(vocab, dtype, precision, topk):
    """The wide path's keys carry 17-bit ids: a wide context at V > 131071 is the library's 'unsupported' error
    (the single-pass configurations at this V run in ``test_coder_matches_oracle``)."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    assert vocab > cv.WIDE_MAX_VOCAB and cv.is_wide(vocab, dtype, topk)
    with pytest.raises(_lib.NativeLibraryError, match="supports vocab < 131072"):
        CoderContext(CoderParams(vocab=vocab, precision=precision, topk=topk, dtype=dtype), max_batch=B)


def test_wide_limit_vocabulary_takes_the_overflow_sweep():
    """V = 131071 at the api defaults (precision 16, topk 50000): the oracle keeps thousands of ranks, about the
    6,144-key LDS budget of the one-pass kernel, so a wave's buffer overflows and the stream takes the block sweep into
    global memory (and the device sort beyond the budget), with ids above 65535.  ``counters()[1]`` counts those
    sweeps on the wide path."""
    from neuralsteganography_amd.coder import CoderContext

    case = next(c for c in CASES if (c.vocab, c.dtype, c.topk) == (cv.WIDE_MAX_VOCAB, "f32", 50000))
    expect = cv.expected(case)
    assert max(tr[0] for e in expect for tr in e.traces) > 5000
    assert any(tok > 65535 for e in expect for tok in e.tokens)
    ctx = CoderContext(_params(case), max_batch=B)
    assert ctx.wide
    rows = _host_rows(lambda s, t: cv.case_row(case, s, t), B, max(len(e.tokens) for e in expect))
    c0 = ctx.counters()
    _run_against_oracle(ctx, rows, case.dtype, expect, alternate_exact=True)
    c1 = ctx.counters()
    assert c1[1] > c0[1], "no stream-step took the overflow sweep"
    assert c1[0] > c0[0], "no stream-step took the exact-sum path"


# ------------------------------------------------------------------------------------------ the row's last ids
# With the default ban list the row's last id (V - 1) is banned, so in the table above the one-id last tile of
# V = 8193 holds no codable id at all.  Here only id 628 is banned and the row's last two ids are its two largest
# logits (rank 0 and 1 of every step's CDF): a kernel that drops, mis-masks or mis-numbers the end of the row -- the
# last tile, the split form's remainder tiles, the wide path's last slice -- shifts every cumulative count.
LAST_SEED = 53
LAST_VOCABS = [65, 771, 8192, 8193, 15871, 16127, 65537, 131071]
LAST_CONFIGS = [("f32", 26, 100), ("f16", 26, 100), ("f32", 16, 50000), ("f16", 22, 2000)]


@functools.lru_cache(maxsize=None)
def _last_ids_reference(vocab, dtype, precision, topk):
    npdt = np.float16 if dtype == "f16" else np.float32

    def row(s, t):
        x = synthetic.logits_row(LAST_SEED, s, t, vocab, 3.0, npdt).astype(np.float32)
        top = x.max()  # (exact in the row's dtype, and so are the two sums below)
        x[vocab - 1], x[vocab - 2] = top + np.float32(0.5), top + np.float32(0.25)
        return x.astype(npdt)

    expect = tuple(cv.oracle_stream(lambda t, s=s: row(s, t), cv.payload_bits(s), banned=[628], temp=0.9,
                                    precision=precision, topk=topk) for s in range(B))
    assert all(vocab - 1 in e.tokens or vocab - 2 in e.tokens for e in expect), "the last ids are never coded"
    return expect, _host_rows(row, B, max(len(e.tokens) for e in expect))


@pytest.mark.parametrize("dtype,precision,topk", LAST_CONFIGS)
@pytest.mark.parametrize("vocab", LAST_VOCABS)
def test_last_ids_of_the_row_are_coded(vocab, dtype, precision, topk):
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    expect, rows = _last_ids_reference(vocab, dtype, precision, topk)
    ctx = CoderContext(CoderParams(vocab=vocab, precision=precision, temp=0.9, topk=topk, dtype=dtype, banned=[628]),
                       max_batch=B)
    assert ctx.wide == cv.is_wide(vocab, dtype, topk, banned=[628])
    _run_against_oracle(ctx, rows, dtype, expect, alternate_exact=ctx.wide)


# ------------------------------------------------------------------------------------------------------ sampler
SAMPLER_VOCABS = [771, 8192, 8193, 16127, 65537, 131071]
SAMPLER_CONFIGS = [("f32", 300, 0.9, 3.0), ("f16", 100, 0.9, 3.0), ("f32", 2000, 1.0, 3.0), ("f32", -1, 1.0, 3.0)]
SAMPLER_L, SAMPLER_SEED, SAMPLER_OFFSET, SAMPLER_ROWS = 12, 0xC0FFEE, 3, 17


def _sampler_row(vocab, dtype, scale, s, t):
    return synthetic.logits_row(SAMPLER_ROWS, s, t, vocab, scale, np.float16 if dtype == "f16" else np.float32)


@functools.lru_cache(maxsize=None)
def _sampler_reference(vocab, dtype, topk, temp, scale):
    out = []
    for s in range(B):
        acc = np.zeros(4)
        ref, _ = oracle.sample_stream(lambda t, s=s: _sampler_row(vocab, dtype, scale, s, t).astype(np.float32),
                                      SAMPLER_L, banned=[vocab - 1, 628], temp=temp, topk=topk, seed=SAMPLER_SEED,
                                      gid=SAMPLER_OFFSET + s, stats=acc)
        out.append((ref, oracle.stats_summary(acc)))
    return out


@pytest.mark.parametrize("dtype,topk,temp,scale", SAMPLER_CONFIGS)
@pytest.mark.parametrize("vocab", SAMPLER_VOCABS)
def test_sampler_matches_oracle(vocab, dtype, topk, temp, scale):
    """``tests/test_gpu_sampler_stats.py::test_sampler_matches_oracle`` off V = 50257, with the poisoned pad: tokens
    bit-exact, statistics within that test's tolerances (rel 1e-4, abs 1e-5: fp32 streaming sums)."""
    from neuralsteganography_amd.coder import CoderContext, CoderParams, sample_batch

    want = _sampler_reference(vocab, dtype, topk, temp, scale)
    ctx = CoderContext(CoderParams(vocab=vocab, precision=26, temp=temp, topk=topk if topk > 0 else vocab,
                                   dtype=dtype), max_batch=B)
    rows = _host_rows(lambda s, t: _sampler_row(vocab, dtype, scale, s, t), B, SAMPLER_L)
    for layout in LAYOUTS:
        toks, stats = sample_batch(ctx, B, SAMPLER_L, _device_rows(rows, dtype, layout), seed=SAMPLER_SEED, topk=topk,
                                   temp=temp, stream_offset=SAMPLER_OFFSET)
        for s in range(B):
            assert toks[s] == want[s][0], f"{layout} stream {s}: sampled tokens differ from the oracle"
            for k in ("avg_NLL", "avg_KL", "avg_Hq"):
                assert stats[s][k] == pytest.approx(want[s][1][k], rel=1e-4, abs=1e-5), (layout, s, k)


# ------------------------------------------------------------------------------------- banned ids at tile edges
BAN_VOCAB, BAN_SEED, BAN_BOOST = 16127, 47, 20.0


def _edge_banned(dtype):
    """[0, TS-1, TS, 2*TS-1, first id of a sample tile, last id of a sample tile, V-1] for the dtype's tile size;
    the sample tiles are tile s*space + space-1 (``_sample_ids`` of ``tests/test_gpu_parity.py``).  fp32: the first
    id of sample tile 1 (read twice by the one-wave form) and the last id of sample tile 8 (kept in registers)."""
    g = geometry(BAN_VOCAB, dtype)
    tiles = [s * g.space + g.space - 1 for s in range(g.nsamp)]
    ban = [0, g.ts - 1, g.ts, 2 * g.ts - 1, tiles[1] * g.ts, (tiles[g.nsamp // 2] + 1) * g.ts - 1, BAN_VOCAB - 1]
    assert len(set(ban)) == 7 and all(0 <= b < BAN_VOCAB for b in ban)
    return ban


@functools.lru_cache(maxsize=None)
def _banned_reference(dtype, precision, topk):
    from neuralsteganography_amd import _lib

    npdt = np.float16 if dtype == "f16" else np.float32
    ban = _edge_banned(dtype)
    assert len(ban) <= _lib.NS_MAX_BANNED

    def row(s, t):  # the banned ids' logits raised before masking: a missed ban changes the token at once
        x = synthetic.logits_row(BAN_SEED, s, t, BAN_VOCAB, 3.0, npdt).astype(np.float32)
        x[ban] += BAN_BOOST
        return x.astype(npdt)

    expect = tuple(cv.oracle_stream(lambda t, s=s: row(s, t), cv.payload_bits(s), banned=ban, temp=0.9,
                                    precision=precision, topk=topk) for s in range(B))
    rows = _host_rows(row, B, max(len(e.tokens) for e in expect))
    for s in range(B):  # with the default ban list alone, step 0 picks one of the raised ids
        _, tok, _ = oracle.encode_step(rows[0, s].astype(np.float32), oracle.new_state(precision),
                                       np.packbits(np.asarray(expect[s].bits, dtype=np.uint8), bitorder="little"),
                                       len(expect[s].bits), banned=[BAN_VOCAB - 1, 628], temp=0.9, precision=precision,
                                       topk=topk)
        assert tok in ban and expect[s].tokens[0] not in ban
    return ban, expect, rows


@pytest.mark.parametrize("dtype,precision,topk", [("f32", 26, 300), ("f16", 26, 100), ("f32", 16, 50000)])
def test_banned_ids_at_tile_edges(dtype, precision, topk):
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    ban, expect, rows = _banned_reference(dtype, precision, topk)
    ctx = CoderContext(CoderParams(vocab=BAN_VOCAB, precision=precision, temp=0.9, topk=topk, dtype=dtype, banned=ban),
                       max_batch=B)
    assert ctx.wide == (topk > 1000)
    if not ctx.wide:
        assert cv.spec_j(BAN_VOCAB, topk, banned=ban) > 0  # the sample is on: the sample tiles' bans are live
    _run_against_oracle(ctx, rows, dtype, expect, alternate_exact=ctx.wide)


# ------------------------------------------------------------------------------- stream quality table off GPT-2
QUALITY_SEED = 43
QUALITY_SETS = {  # (topk, temp, precision) per stream
    "single-pass": [(100, 0.7, 20), (300, 0.9, 26), (512, 1.0, 30)],
    "grouped": [(300, 0.9, 26), (2000, 1.0, 22), (50000, 1.0, 16)],
}


@functools.lru_cache(maxsize=None)
def _quality_reference(vocab, name):
    qs = QUALITY_SETS[name]
    rowf = lambda s, t: synthetic.logits_row(QUALITY_SEED, s, t, vocab, 3.0, np.float32)  # noqa: E731
    expect = tuple(cv.oracle_stream(lambda t, s=s: rowf(s, t), cv.payload_bits(s), banned=[vocab - 1, 628],
                                    temp=q[1], precision=q[2], topk=q[0]) for s, q in enumerate(qs))
    # the streams' own qualities matter: under stream 0's quality the other streams come out differently
    for s in range(1, len(qs)):
        other = cv.oracle_stream(lambda t, s=s: rowf(s, t), cv.payload_bits(s), banned=[vocab - 1, 628],
                                 temp=qs[0][1], precision=qs[0][2], topk=qs[0][0])
        assert other.tokens != expect[s].tokens
    return qs, expect, _host_rows(rowf, len(qs), max(len(e.tokens) for e in expect))


@pytest.mark.parametrize("name", list(QUALITY_SETS))
@pytest.mark.parametrize("vocab", [8193, 131071])
def test_mixed_quality_rows_match_each_streams_own_oracle(vocab, name):
    """``test_mixed_rows_match_the_oracle_of_each_streams_own_quality`` off GPT-2's vocabulary: one mixed call for
    the single-pass qualities (one table), and the front end's grouping (``_quality_groups``: the single-pass
    streams in one table call, one call per wide quality) for {300, 2000, 50000}."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import CoderContext, CoderParams, StreamQuality
    from neuralsteganography_amd.lm.arithmetic import _quality_groups

    qs, expect, rows = _quality_reference(vocab, name)
    plist = [CoderParams(vocab=vocab, precision=q[2], temp=q[1], topk=q[0], dtype="f32") for q in qs]
    groups = _quality_groups(plist, _lib.max_topk(_lib.NS_DTYPE_F32))
    assert groups == ([[0, 1, 2]] if name == "single-pass" else [[0], [1], [2]])
    for g in groups:
        sub = [expect[i] for i in g]
        nmax = max(len(e.tokens) for e in sub)
        if plist[g[0]].topk <= _lib.max_topk(_lib.NS_DTYPE_F32):
            sq = StreamQuality([plist[i] for i in g])
            ctx = CoderContext(sq.context_params(), max_batch=len(g))
            assert not ctx.wide
            _run_against_oracle(ctx, rows[:nmax, g], "f32", sub, quality=sq)
        else:
            ctx = CoderContext(plist[g[0]], max_batch=len(g))
            assert ctx.wide
            _run_against_oracle(ctx, rows[:nmax, g], "f32", sub, alternate_exact=True)
