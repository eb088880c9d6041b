"""GPU: the decode step's divergence report, rank export and re-issue (``ns_decode_step`` with ``d_trace`` and
``ns_set_rank_export``, raw ctypes) against the oracle runs of ``tests/decode_diverge_cases.py``, which
``tests/test_decode_diverge_host.py`` checks on the CPU.  The contract under test is the one ``include/nsg_coder.h``
states under "Divergence contract".

Every comparison is exact (integers, bytes, id lists).  Before every call the trace and export arrays hold a sentinel
(-7) in every element, and the output rows hold a byte pattern in every bit at or beyond the stream's ``bit_pos`` (the
kernel writes bit by bit, so the pattern survives wherever nothing was emitted; the whole row is compared).  Pad
columns ``[V, ld)`` of every row are poisoned as in ``tests/test_gpu_coder_vocab.py``.

Forms: the wide families assert ``ctx.wide``; the sweep family asserts ``counters()[1]`` rising; the single-pass
families run with ``ns_set_split_max_batch`` 0 (one wave per stream) and 2^30 (split form) and assert the setter
reports the value just set -- the kernel takes the split form only where the stratified sample is on (the 'sample'
family), elsewhere the switch selects nothing and both runs are the wave form.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from tests import coder_vocab_cases as cv
from tests import decode_diverge_cases as dd
from tests.decode_diverge_cases import B, CASES

pytestmark = pytest.mark.gpu

SENTINEL = -7
PATTERN = 0xA5
TMAX = 14
ERR_BITS = 1 | 2 | 4   # NS_ST_DONE | NS_ST_ERR_RANGE | NS_ST_ERR_DIVERGE (NS_ST_EXACT_SUM is a diagnostic)
DIVERGED = 4 | 1
RANGE = 2 | 1


def _torch():
    import torch

    return torch


def _poison(s, npdt):
    return (np.nan, np.inf, float(np.finfo(npdt).max))[s % 3]


@functools.lru_cache(maxsize=None)
def _context(vocab, dtype, topk, precision, temp, quality):
    """One coder context per family member (both variants and both forms share it)."""
    from neuralsteganography_amd.coder import CoderContext, CoderParams, StreamQuality

    if quality:
        sq = StreamQuality([CoderParams(vocab=vocab, precision=q[2], temp=q[1], topk=q[0], dtype=dtype)
                            for q in dd.QUALITIES])
        return CoderContext(sq.context_params(), max_batch=B), sq
    return CoderContext(CoderParams(vocab=vocab, precision=precision, temp=temp, topk=topk, dtype=dtype),
                        max_batch=B), None


@functools.lru_cache(maxsize=4)
def _device_rows(case):
    """[TMAX, B, ld] device rows of ``case``, pads poisoned by stream."""
    torch = _torch()
    host = np.empty((TMAX, B, case.ld), case.npdt)
    for s in range(B):
        host[:, s, :] = _poison(s, case.npdt)
        for t in range(TMAX):
            host[t, s, : case.vocab] = dd.case_row(case, s, t)
    return torch.from_numpy(host).cuda()


def _expected_row(oracle_bytes, bit_pos, nbytes):
    """The output row the kernel must leave: the oracle's bits below ``bit_pos``, the pattern from there on."""
    bits = np.unpackbits(np.full(nbytes, PATTERN, np.uint8), bitorder="little")
    bits[:bit_pos] = np.unpackbits(np.frombuffer(oracle_bytes, dtype=np.uint8), bitorder="little")[:bit_pos]
    return np.packbits(bits, bitorder="little")


class Runner:
    """The device arrays of one decode run and the raw ``ns_decode_step`` call."""

    def __init__(self, case, stride=None):
        from neuralsteganography_amd import _lib
        from neuralsteganography_amd.coder import _ptr, _stream_handle, _table_registered

        torch = _torch()
        self.case = case
        self.ctx, self.sq = _context(case.vocab, case.dtype, case.topk, case.precision, case.temp,
                                    case.family == "quality")
        self.L, self._lib, self._ptr, self._stream = _lib.lib(), _lib, _ptr, _stream_handle
        dev = torch.device("cuda", self.ctx.device)
        self.dev = dev
        self.table = self.sq.table(dev) if self.sq is not None else None
        self._reg = lambda: _table_registered(self.ctx, self.table, self.sq.k_max if self.sq else 0)
        self.out_stride = dd.out_bytes(case) + 3
        self.out = torch.full((B + 1, self.out_stride), PATTERN, dtype=torch.uint8, device=dev)  # + a guard row
        self.state = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        with self._reg():
            self.ctx.check(self.L.ns_init_state(self.ctx._h, _ptr(self.state), B, _stream_handle()), "ns_init_state")
        self.trace = torch.empty((B + 1, 8), dtype=torch.int32, device=dev)
        self.stride = int(self.ctx.K) + 1 if stride is None else int(stride)
        self.ranked = torch.empty(B * self.stride + 64, dtype=torch.int32, device=dev)  # + guard elements
        self.rows = _device_rows(case)

    def load(self, states, out_rows):
        """Set every stream's state (lo, hi, bit_pos, ntokens; flags 0) and output row from host values."""
        torch = _torch()
        st = np.zeros((B, 4), dtype=np.uint64)
        for s, (lo, hi, bp, nt) in enumerate(states):
            st[s] = (lo, hi, bp, nt)
        self.state.copy_(torch.from_numpy(st.view(np.int64)))
        self.out[:B].copy_(torch.from_numpy(np.stack(out_rows)))

    def clear(self, streams):
        w = self.state.view(_torch().int32)
        for s in streams:
            w[s, 7] = w[s, 7] & ~(self._lib.NS_ST_ERR_DIVERGE | self._lib.NS_ST_DONE)

    def step(self, logits, tokens, last, active=None, export=True):
        """Sentinels into the trace and export arrays, then one ``ns_decode_step``."""
        torch = _torch()
        p = self.ctx.params
        self.trace.fill_(SENTINEL)
        self.ranked.fill_(SENTINEL)
        tok = torch.tensor(np.asarray(tokens, dtype=np.int32), device=self.dev)
        lst = torch.tensor(np.asarray(last, dtype=np.uint8), device=self.dev)
        act = torch.tensor(np.asarray(active, dtype=np.uint8), device=self.dev) if active is not None else None
        assert logits.shape == (B, self.case.ld) and logits.is_contiguous()
        if export:
            self.ctx.check(self.L.ns_set_rank_export(self.ctx._h, self._ptr(self.ranked), self.stride),
                           "ns_set_rank_export")
        with self._reg():
            rc = self.L.ns_decode_step(self.ctx._h, self._ptr(logits), self.case.ld, B, self._ptr(tok), self._ptr(lst),
                                       self._ptr(act), self._ptr(self.state), self._ptr(self.out), self.out_stride,
                                       float(p.temp), int(p.topk), self.ctx._banned, self.ctx._nbanned,
                                       self._ptr(self.trace), 0, self._stream())
        self.L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, "ns_decode_step")
        torch.cuda.synchronize()

    def snap(self):
        st = self.state.cpu().numpy()
        u = st.view(np.uint64)
        w = st.view(np.int32).reshape(B, 8)
        return {"state": [(int(u[s, 0]), int(u[s, 1]), int(st[s, 2]), int(w[s, 6])) for s in range(B)],
                "flags": [int(w[s, 7]) & ERR_BITS for s in range(B)],
                "out": self.out.cpu().numpy(),
                "trace": [tuple(int(v) for v in r[:5]) for r in self.trace.cpu().numpy()],
                "ranked": self.ranked.cpu().numpy()}

    def expected_export(self, kept_by_stream):
        """The whole export array: ``(kept + [-1])[:stride]`` in the row of every stream of ``kept_by_stream``, the
        sentinel everywhere else (the rest of those rows, the other streams' rows, the guard elements)."""
        want = np.full(self.ranked.numel(), SENTINEL, np.int32)
        for s, kept in kept_by_stream.items():
            ids = (list(kept) + [-1])[: self.stride]
            want[s * self.stride: s * self.stride + len(ids)] = ids
        return want


NO_TRACE = (SENTINEL,) * 5


def _check_guards(got, run):
    assert (got["out"][B] == PATTERN).all(), "a write past the last stream's output row"
    assert got["trace"][B] == NO_TRACE, "a write past the last stream's trace"


@pytest.fixture(params=["wave", "split"])
def coder_form(request):
    """The single-pass forms: one wave per stream, and the split form forced at every batch size."""
    from neuralsteganography_amd import _lib

    want = 0 if request.param == "wave" else 1 << 30
    prev = _lib.set_split_max_batch(want)
    assert _lib.set_split_max_batch(want) == want, "ns_set_split_max_batch does not report the value just set"
    yield request.param
    assert _lib.set_split_max_batch(prev) == want


def _run_case(case):
    """The whole protocol on one case: every stream meets its bad token once, is skipped while flagged, is cleared
    and re-issued alone, and the run goes on to the end."""
    exp = dd.expected(case)
    run = Runner(case)
    assert run.ctx.wide == case.family.startswith("wide")
    assert run.stride == min(case.topk, cv.nvalid(case.vocab, case.banned)) + 1
    nb = run.out_stride
    T = [len(e.tokens) for e in exp]
    zero = bytes(dd.out_bytes(case))

    def after(s, t):  # oracle state / bytes after stream s has decoded tokens 0 .. t-1
        e = exp[s]
        st = e.steps[t].state if t < T[s] else e.final
        return st, _expected_row(e.steps[t - 1].out if t else zero, st[2], nb)

    done = [0] * B  # tokens decoded so far
    for t in range(TMAX):
        active = [t < T[s] for s in range(B)]
        bad = [s for s in range(B) if active[s] and exp[s].bad_step == t]
        tokens = [0 if not active[s] else exp[s].bad_token if s in bad else exp[s].tokens[t] for s in range(B)]
        last = [active[s] and t == T[s] - 1 for s in range(B)]
        run.step(run.rows[t], tokens, last, active)
        got = run.snap()
        _check_guards(got, run)
        for s in range(B):
            if active[s] and s not in bad:
                done[s] += 1
            st, row = after(s, done[s])
            what = f"step {t} stream {s} ({exp[s].cls})"
            assert got["state"][s] == st, f"{what}: state"
            assert np.array_equal(got["out"][s], row), f"{what}: output bytes"
            if not active[s]:
                assert got["flags"][s] == 0 and got["trace"][s] == NO_TRACE, what
            elif s in bad:
                k, kp = exp[s].steps[t].trace[:2]
                assert got["flags"][s] == DIVERGED, f"{what}: flags {got['flags'][s]}"
                assert got["trace"][s] == (k, kp, -1, -1, -1), f"{what}: trace {got['trace'][s]}"
            else:
                assert got["flags"][s] == 0, f"{what}: flags {got['flags'][s]}"
                assert got["trace"][s] == exp[s].steps[t].trace, f"{what}: trace {got['trace'][s]}"
        want = run.expected_export({s: exp[s].steps[t].kept for s in bad})
        diff = np.nonzero(got["ranked"] != want)[0]
        assert diff.size == 0, f"step {t}: export differs at elements {diff[:8].tolist()} (stride {run.stride})"
        if not bad:
            continue
        # still flagged: a second step with the clean token skips the stream
        only = [s in bad for s in range(B)]
        clean = [exp[s].tokens[t] if s in bad else 0 for s in range(B)]
        run.step(run.rows[t], clean, last, only)
        again = run.snap()
        _check_guards(again, run)
        assert again["state"] == got["state"] and again["flags"] == got["flags"], f"step {t}: a flagged stream ran"
        assert np.array_equal(again["out"], got["out"]), f"step {t}: a flagged stream wrote bits"
        assert all(tr == NO_TRACE for tr in again["trace"]), f"step {t}: a flagged stream wrote its trace"
        assert (again["ranked"] == SENTINEL).all(), f"step {t}: a flagged stream wrote the export"
        # cleared and re-issued alone
        run.clear(bad)
        run.step(run.rows[t], clean, last, only)
        redo = run.snap()
        _check_guards(redo, run)
        assert (redo["ranked"] == SENTINEL).all(), f"step {t}: the re-issue wrote the export"
        for s in range(B):
            what = f"re-issue of step {t}, stream {s} ({exp[s].cls})"
            if s in bad:
                done[s] += 1
                st, row = after(s, done[s])
                assert redo["flags"][s] == 0 and redo["state"][s] == st, f"{what}: state"
                assert np.array_equal(redo["out"][s], row), f"{what}: output bytes"
                assert redo["trace"][s] == exp[s].steps[t].trace, f"{what}: trace {redo['trace'][s]}"
                if exp[s].cls == "g":  # nothing on the diverged step, all P bits of the new bottom now
                    assert last[s] and redo["state"][s][2] - got["state"][s][2] == case.quality(s)[2], what
            else:
                assert redo["state"][s] == got["state"][s] and redo["flags"][s] == got["flags"][s], f"{what}: state"
                assert np.array_equal(redo["out"][s], got["out"][s]), f"{what}: output bytes"
                assert redo["trace"][s] == NO_TRACE, f"{what}: trace"
    final = run.snap()
    for s in range(B):
        assert done[s] == T[s] and final["state"][s] == exp[s].final and final["flags"][s] == 0
        bits = np.unpackbits(final["out"][s], bitorder="little")[: exp[s].final[2]].tolist()
        assert bits == exp[s].decoded, f"stream {s}: decoded bits differ from the oracle's"
    return run


SINGLE = [c for c in CASES if c.family in dd.SINGLE_PASS_FAMILIES]
WIDE = [c for c in CASES if c.family == "wide-lds"]
SWEEP = [c for c in CASES if c.family == "wide-sweep"]


@pytest.mark.parametrize("case", SINGLE, ids=[c.id for c in SINGLE])
def test_single_pass_divergence_and_reissue(case, coder_form):
    run = _run_case(case)
    assert not run.ctx.wide
    assert cv.sample_on(case.vocab, case.dtype, case.topk) == (case.family == "sample")
    assert (run.sq is not None) == (case.family == "quality")


@pytest.mark.parametrize("case", WIDE, ids=[c.id for c in WIDE])
def test_wide_lds_divergence_and_reissue(case):
    run = _run_case(case)
    assert run.ctx.wide


@pytest.mark.parametrize("case", SWEEP, ids=[c.id for c in SWEEP])
def test_wide_sweep_divergence_and_reissue(case):
    ctx, _ = _context(case.vocab, case.dtype, case.topk, case.precision, case.temp, False)
    c0 = ctx.counters()
    run = _run_case(case)
    assert run.ctx is ctx and ctx.wide
    assert ctx.counters()[1] > c0[1], "no stream-step went beyond the LDS key budget"


# ------------------------------------------------------------------------------------------------ one-step probes
# Every stream is put at the oracle's state before its own bad step (its row of that step, its bytes so far) and
# receives one token; the outcome is the oracle's for that token from that state.
PROBED = [next(c for c in CASES if (c.family, c.dtype, c.variant) == (f, "f32", v))
          for f in ("single", "sample", "quality", "wide-lds", "wide-sweep") for v in (0, 1)]
STRIDED = [next(c for c in CASES if (c.family, c.vocab, c.dtype, c.variant) == k)
           for k in (("single", 1025, "f32", 0), ("wide-lds", 1025, "f32", 0))]


def _probe_rows(run, exp, rows_host=None):
    torch = _torch()
    if rows_host is None:
        return torch.stack([run.rows[exp[s].bad_step, s] for s in range(B)]).contiguous()
    return torch.from_numpy(rows_host).cuda()


def _probe(run, tokens, *, export=True, logits=None):
    """Load the pre-bad-step states, decode ``tokens`` (one per stream) and compare with the oracle's outcome."""
    from oracle import oracle

    case, exp = run.case, dd.expected(run.case)
    nb = run.out_stride
    zero = bytes(dd.out_bytes(case))
    before = []
    for s in range(B):
        bt = exp[s].bad_step
        before.append(_expected_row(exp[s].steps[bt - 1].out if bt else zero, exp[s].steps[bt].state[2], nb))
    run.load([exp[s].steps[exp[s].bad_step].state for s in range(B)], before)
    last = [exp[s].bad_step == len(exp[s].tokens) - 1 for s in range(B)]
    run.step(_probe_rows(run, exp) if logits is None else logits, tokens, last, None, export=export)
    got = run.snap()
    _check_guards(got, run)
    kept = {}
    for s in range(B):
        rc, st, tr, ids, out = dd.oracle_try(case, s, exp[s].bad_step, tokens[s])
        what = f"stream {s} token {tokens[s]}"
        assert got["state"][s] == st and got["trace"][s] == tr, f"{what}: {got['state'][s]} {got['trace'][s]}"
        assert np.array_equal(got["out"][s], _expected_row(out, st[2], nb)), f"{what}: output bytes"
        assert got["flags"][s] == (0 if rc == oracle.OR_OK else DIVERGED), what
        if rc != oracle.OR_OK:
            kept[s] = ids
    return got, kept


@pytest.mark.parametrize("case", PROBED, ids=[c.id for c in PROBED])
def test_controls_decode_and_nothing_is_exported(case, coder_form):
    """The ids at rank k' - 1 and rank 0 of every stream's bad step decode as the oracle does and leave the export
    array alone.  (The form switch only matters to the single-pass cases.)"""
    run = Runner(case)
    exp = dd.expected(case)
    for which in (0, 1):
        got, kept = _probe(run, [exp[s].controls[which] for s in range(B)])
        assert not kept and (got["ranked"] == SENTINEL).all()


@pytest.mark.parametrize("case", STRIDED, ids=[c.id for c in STRIDED])
def test_export_stride_variants(case):
    """Streams 0, 2, 4 receive their bad token, streams 1, 3, 5 their clean one, with the export at stride K + 1, at
    stride = stream 0's k' (k' ids, no terminator), at stride 5 (five ids; the next stream's row untouched), and
    switched off; stride 1 is refused."""
    from neuralsteganography_amd import _lib

    exp = dd.expected(case)
    tokens = [exp[s].bad_token if s % 2 == 0 else exp[s].tokens[exp[s].bad_step] for s in range(B)]
    kps = [exp[s].steps[exp[s].bad_step].trace[1] for s in range(B)]
    assert kps[0] > 5 and len({kps[0], kps[2], kps[4]}) > 1  # truncated, exact and terminated rows all occur
    for stride in (None, kps[0], 5):
        run = Runner(case, stride=stride)
        got, kept = _probe(run, tokens)
        assert sorted(kept) == [0, 2, 4]
        want = run.expected_export(kept)
        if stride == kps[0]:
            assert want[0: stride].tolist() == list(kept[0]) and -1 not in want[:stride].tolist()
        if stride == 5:
            assert want[5] == SENTINEL and want[:5].tolist() == list(kept[0][:5])
        diff = np.nonzero(got["ranked"] != want)[0]
        assert diff.size == 0, f"stride {run.stride}: export differs at elements {diff[:8].tolist()}"
    run = Runner(case)
    got, kept = _probe(run, tokens, export=False)  # the flags are checked by _probe
    assert sorted(kept) == [0, 2, 4] and (got["ranked"] == SENTINEL).all()
    for stride in (1, 0, -3):
        rc = run.L.ns_set_rank_export(run.ctx._h, run._ptr(run.ranked), stride)
        assert rc == _lib.NS_ERR_CONFIG, f"stride {stride} accepted"
    run.L.ns_set_rank_export(run.ctx._h, ctypes.c_void_p(0), 0)


@pytest.mark.parametrize("case", STRIDED, ids=[c.id for c in STRIDED])
def test_non_finite_row_is_a_range_error_without_export(case):
    """Stream 0's row is NaN throughout, stream 1's has one +inf logit, both with a token that diverges on the
    finite row: NS_ST_ERR_RANGE and not NS_ST_ERR_DIVERGE, state and bits unchanged, no export -- on both paths.
    Stream 2 diverges next to them and is exported as usual; stream 3 decodes."""
    exp = dd.expected(case)
    run = Runner(case)
    host = _probe_rows(run, exp).cpu().numpy().copy()
    host[0, : case.vocab] = np.nan
    host[1, 17] = np.inf
    tokens = [exp[s].bad_token if s < 3 else exp[s].tokens[exp[s].bad_step] for s in range(B)]
    assert all(0 <= tokens[s] < case.vocab and tokens[s] not in case.banned for s in (0, 1)) and tokens[1] != 17
    nb = run.out_stride
    zero = bytes(dd.out_bytes(case))
    before = []
    for s in range(B):
        bt = exp[s].bad_step
        before.append(_expected_row(exp[s].steps[bt - 1].out if bt else zero, exp[s].steps[bt].state[2], nb))
    states = [exp[s].steps[exp[s].bad_step].state for s in range(B)]
    run.load(states, before)
    run.step(_probe_rows(run, exp, host), tokens, [False] * B, None)
    got = run.snap()
    _check_guards(got, run)
    for s in (0, 1):
        assert got["flags"][s] == RANGE, f"stream {s}: flags {got['flags'][s]}"
        assert got["state"][s] == states[s] and np.array_equal(got["out"][s], before[s])
        assert got["trace"][s][2:] == (-1, -1, -1) or got["trace"][s] == NO_TRACE
    assert got["flags"][2] == DIVERGED and got["flags"][3] == 0 and got["state"][3][3] == states[3][3] + 1
    want = run.expected_export({2: exp[2].steps[exp[2].bad_step].kept})
    diff = np.nonzero(got["ranked"] != want)[0]
    assert diff.size == 0, f"export differs at elements {diff[:8].tolist()}"


@pytest.mark.parametrize("case", [WIDE[0], SWEEP[0]], ids=[WIDE[0].id, SWEEP[0].id])
def test_ranked_ids_of_a_wide_streaming_session(case):
    """``StreamingDecodeSession.ranked_ids`` on a wide context (``rank_stride`` = K + 1): the oracle's kept ids of
    every stream that diverged on its first token; cleared and re-issued, the clean token decodes."""
    from neuralsteganography_amd.coder import StreamingDecodeSession
    from oracle import oracle

    exp = dd.expected(case)
    ctx, _ = _context(case.vocab, case.dtype, case.topk, case.precision, case.temp, False)
    assert ctx.wide
    sess = StreamingDecodeSession(ctx, B, max_tokens=TMAX)
    assert sess.rank_stride == cv.nvalid(case.vocab, case.banned) + 1
    rows = _device_rows(case)
    low = [int(dd.numpy_order(dd.case_row(case, s, 0), case.banned)[-1]) for s in range(B)]
    tokens = [low[s] if s % 2 == 0 else exp[s].tokens[0] for s in range(B)]
    sess.step(rows[0], tokens, [False] * B, [True] * B)
    assert sess.diverged() == [0, 2, 4]
    for s in (0, 2, 4):
        rc, _, _, kept, _ = dd.oracle_try(case, s, 0, low[s], is_last=False)
        assert rc == oracle.OR_ERR_DIVERGE and sess.ranked_ids(s) == list(kept) == list(exp[s].steps[0].kept)
    sess.clear([0, 2, 4])
    sess.step(rows[0], [exp[s].tokens[0] for s in range(B)], [False] * B, [s % 2 == 0 for s in range(B)])
    assert sess.diverged() == []
    for s, bits in enumerate(sess.bits()):
        n = exp[s].steps[1].state[2]
        assert bits == np.unpackbits(np.frombuffer(exp[s].steps[0].out, np.uint8), bitorder="little")[:n].tolist()
