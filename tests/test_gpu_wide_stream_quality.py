"""GPU: one coder quality (temperature, top-k, precision) per stream on the WIDE path -- a table registered with
``ns_set_stream_quality_wide`` whose ``k_max`` is beyond the single-pass limit (``ns_max_topk``), so that the step runs
``wide_onepass_kernel`` -> device sort -> ``wide_cdf_kernel`` and each of them reads stream ``b``'s row.

The contract is that of ``tests/test_gpu_stream_quality.py``: a stream's tokens, bits and step traces are those of a
call with that stream's quality alone.  Every comparison is exact (token lists, bit lists, trace integers, state
bytes) against the CPU oracle run with the stream's own (temp, precision, topk) or against the scalar wide call; the
statistics keep the project's bound (rel 2e-5, abs 2e-6).  The fixture checks that at least 6 of the 8 streams come
out differently under row 2's quality (the api default), so a kernel that applied one quality to every stream could
not pass.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.coder import (CoderContext, CoderParams, DecodeSession, EncodeSession,  # noqa: E402
                                           SampleSession, StreamQuality, row_stride)
from neuralsteganography_amd.exceptions import ConfigurationError  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

V, B, SEED, SCALE, NSTEP = 50257, 8, 31, 3.0, 24  # one launch of eight rows
NBYTES = 64  # payload per stream: more than any row consumes in 24 steps (at most 282 of the 512 bits)
BANNED = [V - 1, 628]
API_DEFAULT = (50000, 1.0, 16)


def _limit(dtype):
    return _lib.max_topk(_lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32)


def _qualities(dtype):
    """(topk, temp, precision) per stream; kept keys = ids the one-pass kernel collects, over the 24 steps."""
    return [(_limit(dtype) + 1, 0.9, 26),  # the 1/R cutoff never binds: k stays at limit + 1
            (5000, 0.7, 16),               # LDS tail, 20-1,445 keys kept
            API_DEFAULT,                   # LDS tail, 71-4,280 keys kept
            (50000, 1.3, 22),              # up to 39,044 keys: wave-buffer overflow sweep, device sort, list kernel
            (60000, 1.0, 40),              # 50,084-50,255 keys: list kernel, K = every valid id
            (2, 1.0, 12),                  # narrow rows in a wide launch: K only shortens the ranks looked at
            (300, 0.9, 26),
            (50000, 0.8, 12)]              # LDS tail, 2-403 keys kept


def _params(dtype, q):
    return CoderParams(vocab=V, precision=q[2], temp=q[1], topk=q[0], dtype=dtype)


def _oracle(dtype, s, bits, q):
    """NSTEP oracle encode steps of stream s under quality q: tokens, (k, k', sel, n, token) traces, final bit_pos."""
    npdt = np.float16 if dtype == "f16" else np.float32
    packed = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    st = oracle.new_state(q[2])
    toks, traces = [], []
    for t in range(NSTEP):
        row = synthetic.logits_row(SEED, s, t, V, SCALE, npdt).astype(np.float32)
        rc, tok, tr = oracle.encode_step(row, st, packed, len(bits), banned=BANNED, temp=q[1], precision=q[2],
                                         topk=q[0])
        assert rc == 0 and st.bit_pos < len(bits)
        toks.append(tok)
        traces.append((tr.k, tr.kprime, tr.sel, tr.n, tr.token))
    return toks, traces, int(st.bit_pos)


@functools.lru_cache(maxsize=None)
def _reference(dtype):
    """Per dtype, computed once on the CPU: the payloads and the oracle's tokens and traces of every stream under its
    OWN quality -- and the check that one quality for all (row 2's) would give other tokens."""
    qs = _qualities(dtype)
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(900 + s, NBYTES)) for s in range(B)]
    expect = [_oracle(dtype, s, bits[s], qs[s]) for s in range(B)]
    assert all(tr[0] == qs[0][0] for tr in expect[0][1]), "row 0: the cutoff binds"
    assert all(tr[0] <= 2 for tr in expect[5][1]) and all(tr[0] <= 300 for tr in expect[6][1])
    under_one = [_oracle(dtype, s, bits[s], qs[2])[0] for s in range(B)]
    assert sum(a != e[0] for a, e in zip(under_one, expect)) >= 6, "row 2's quality gives the same tokens"
    return qs, bits, expect


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """:func:`_reference` plus the 24 logit matrices on the device and the quality rows."""
    qs, bits, expect = _reference(dtype)
    npdt = np.float16 if dtype == "f16" else np.float32
    ld = row_stride(V, dtype)
    rows = [torch.from_numpy(synthetic.logits_batch(SEED, range(B), t, V, SCALE, npdt, ld)).cuda()
            for t in range(NSTEP)]
    sq = StreamQuality([_params(dtype, q) for q in qs])
    assert sq.k_max == 60000
    return dtype, qs, bits, expect, rows, sq


@pytest.fixture(params=["f32", "f16"])
def case(request):
    return _case(request.param)


def _run_encode(ctx, bits, rows, sq, expect=None, stats=False, **step_kw):
    sess = EncodeSession(ctx, bits, quality=sq, stats=stats)
    sess.enable_trace()
    for t in range(NSTEP):
        sess.step(rows[t], **step_kw)
        if expect is not None:
            tr = sess.trace_rows()
            for s in range(len(bits)):
                got = (int(tr.k[s]), int(tr.kprime[s]), int(tr.sel[s]), int(tr.n[s]), int(tr.token[s]))
                assert got == expect[s][1][t], f"stream {s} step {t}: kernel {got} oracle {expect[s][1][t]}"
    f = sess.fields()
    assert not (f["flags"] & (_lib.NS_ST_DONE | _lib.NS_ST_ERR_RANGE | _lib.NS_ST_ERR_DIVERGE)).any()
    if expect is not None:
        assert f["bit_pos"].tolist() == [e[2] for e in expect]
    return sess


def _decode(ctx, toks, rows, sq):
    dec = DecodeSession(ctx, toks, quality=sq)
    for t in range(dec.T):
        dec.step(rows[t])
    return dec.bits()


def test_mixed_rows_match_the_oracle_of_each_streams_own_quality(case):
    dtype, qs, bits, expect, rows, sq = case
    ctx = CoderContext(sq.context_params(), max_batch=B)
    assert ctx.wide
    before = ctx.counters()
    sess = _run_encode(ctx, bits, rows, sq, expect)
    toks = sess.tokens()
    assert toks == [e[0] for e in expect]
    # both tails ran: a wave buffer overflowed (rows 3 and 4 keep tens of thousands of keys), so the block sweep,
    # the device sort and the list kernel served those streams while fast_tail served the others
    assert ctx.counters()[1] > before[1]
    hi = sess.fields()["hi"]
    assert all(int(hi[s]) <= 1 << qs[s][2] for s in range(B))
    out = _decode(ctx, toks, rows, sq)
    for s in range(B):
        # every token but the last gives back the n payload bits it fixed; the last one emits all `precision` bits
        # of the interval's bottom -- the precision of this stream's row
        fixed = sum(tr[3] for tr in expect[s][1][:-1])
        assert fixed >= 8 and len(out[s]) == fixed + qs[s][2], s
        assert out[s][:fixed] == bits[s][:fixed], f"stream {s}: decoded bits differ from the payload"


def test_equal_rows_give_the_scalar_wide_calls_outputs(case):
    dtype, _, bits, _, rows, _ = case
    p = _params(dtype, API_DEFAULT)
    ctx = CoderContext(p, max_batch=B)
    assert ctx.wide
    outs = []
    for sq in (None, StreamQuality([p] * B)):
        sess = EncodeSession(ctx, bits, quality=sq)
        sess.enable_trace()
        traces = []
        for t in range(NSTEP):
            sess.step(rows[t])
            traces.append(sess.trace.cpu().numpy().copy())
        outs.append((sess.tokens(), np.stack(traces), sess.state.cpu().numpy(), _decode(ctx, sess.tokens(), rows, sq)))
    assert outs[0][0] == outs[1][0] and outs[0][3] == outs[1][3]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_forced_exact_sum_with_a_wide_table():
    dtype, qs, bits, expect, rows, sq = _case("f32")
    ctx = CoderContext(sq.context_params(), max_batch=B)
    before = ctx.counters()
    sess = _run_encode(ctx, bits, rows, sq, expect, force_exact=True)
    assert sess.tokens() == [e[0] for e in expect]
    assert ctx.counters()[0] - before[0] >= B * NSTEP  # every stream-step summed its row exactly, at its own temp


def test_statistics_with_a_wide_table_match_each_stream_alone():
    """Each stream's statistics against the scalar call with that stream's quality and that stream alone (the wide
    chain for rows beyond the single-pass limit, the single-pass kernel for rows 5 and 6)."""
    dtype, qs, bits, expect, rows, sq = _case("f16")
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _run_encode(ctx, bits, rows, sq, expect, stats=True)
    assert sess.tokens() == [e[0] for e in expect]
    got = sess.stats()
    for s in range(B):
        alone = EncodeSession(CoderContext(_params(dtype, qs[s]), max_batch=1), [bits[s]], stats=True)
        for t in range(NSTEP):
            alone.step(rows[t][s:s + 1])
        assert alone.tokens() == [expect[s][0]]
        for k, v in alone.stats()[0].items():
            assert got[s][k] == pytest.approx(v, rel=2e-5, abs=2e-6), (s, k)


def test_the_wide_entry_refuses_what_it_cannot_serve(case):
    dtype, qs, bits, _, rows, sq = case
    L = _lib.lib()
    limit = _limit(dtype)
    table = sq.table(torch.device("cuda", 0))
    narrow = CoderContext(CoderParams(vocab=V, precision=26, topk=300, dtype=dtype), max_batch=B)
    assert L.ns_set_stream_quality_wide(narrow._h, table.data_ptr(), sq.k_max) == _lib.NS_ERR_UNSUPPORTED
    ctx = CoderContext(sq.context_params(), max_batch=B)
    assert L.ns_set_stream_quality_wide(ctx._h, table.data_ptr(), 0) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality_wide(ctx._h, table.data_ptr() + 4, sq.k_max) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality_wide(None, table.data_ptr(), sq.k_max) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality(ctx._h, table.data_ptr(), limit + 1) == _lib.NS_ERR_UNSUPPORTED  # the old entry
    smp = SampleSession(ctx, B, seed=1, topk=40, temp=1.0, max_tokens=2, stats=False)
    assert L.ns_set_stream_quality_wide(ctx._h, table.data_ptr(), sq.k_max) == _lib.NS_OK
    try:
        with pytest.raises(ConfigurationError):
            smp.step(rows[0])
    finally:
        assert L.ns_set_stream_quality_wide(ctx._h, None, 0) == _lib.NS_OK
    smp.step(rows[0])  # cleared: the sampler runs again
    torch.cuda.synchronize()
