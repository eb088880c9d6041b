"""GPU: the src rank coder (``ns_rank_encode_step`` / ``ns_rank_decode_step`` / ``ns_token_probs``: wide_stats_kernel,
wide_collect_kernel, the device sort, wide_rank_kernel over fp32 and fp16 rows, wide_rank64_kernel over provider rows)
against the CPU oracle across vocabulary sizes, dtypes, quality policies and row strides.

Bar: at every step the kernel's trace (n, c, sel, bits taken or kept, token) equals the oracle's -- the support size n
included, which the coder itself uses only through c = floor(log2 n) -- and so do the final tokens, the consumption
history, the per-stream status and the decoded payloads.  The oracle runs are those of ``tests/rank_vocab_cases.py``,
which ``tests/test_rank_vocab_host.py`` checks on the CPU (against a numpy restatement of the reference's formulas).
The oracle sees ``row[:V]`` only; the kernel sees the two layouts of ``tests/test_gpu_coder_vocab.py`` with their
poisoned pad columns (NaN, +inf, the dtype's largest finite value per stream).
"""

from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest

from neuralsteganography_amd import synthetic
from oracle import oracle
from tests import rank_vocab_cases as rv
from tests.rank_vocab_cases import B, CASES, PROVIDER_CASES
from tests.test_gpu_coder_vocab import LAYOUTS, _device_rows, _host_rows
from tests.test_rank_vocab_host import numpy_support

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _ctx(vocab, dtype, max_batch=B):
    """One rank context per (V, dtype), as ``HipRankLM`` creates it (no banned ids, every id ranked)."""
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    return CoderContext(CoderParams(vocab=vocab, precision=16, temp=1.0, topk=vocab, dtype=dtype, banned=[]),
                        max_batch=max_batch)


def _status(flags):
    from neuralsteganography_amd import _lib

    out = []
    for f in flags.tolist():
        if f & _lib.NS_ST_ERR_RANGE:
            out.append("range")
        elif f & _lib.NS_ST_ERR_DIVERGE:
            out.append("diverge")
        else:
            out.append("done" if f & _lib.NS_ST_DONE else "open")
    return out


def _trace(sess):
    """The last step's (n, c, sel, bits, token) per stream."""
    tr = sess.trace_rows()
    return [(int(tr.k[s]), int(tr.kprime[s]), int(tr.sel[s]), int(tr.n[s]), int(tr.token[s])) for s in range(sess.B)]


def _encoded(sess):
    """(tokens, consumption) per stream, also of the streams in error (``tokens()`` raises for those)."""
    n = sess.fields()["ntokens"]
    h, c = sess.hist.cpu().numpy(), sess.cons.cpu().numpy()
    return ([h[i, : int(n[i])].tolist() for i in range(sess.B)], [c[i, : int(n[i])].tolist() for i in range(sess.B)])


def _decoded(dec):
    """The whole bytes every stream has emitted, also of the streams in error (``payloads()`` raises for those)."""
    from neuralsteganography_amd.coder import _state_fields

    f = _state_fields(dec.state)
    ob = dec.out_bits.cpu().numpy()
    return [ob[i, : int(f["bit_pos"][i]) // 8].tobytes() for i in range(dec.B)], _status(f["flags"])


def _nsteps(expect):
    return max(len(e.steps) + (e.status == "range") for e in expect)


def _run_against_oracle(ctx, expect, step_rows, *, temp, quality, vocab=None, label="", totals=None):
    """Encode ``expect``'s payloads step by step on ``step_rows(t)`` against the oracle's (n, c, sel, take, token);
    then decode the tokens with their histories against the oracle's (n, c, sel, keep, token).  ``totals(s, t)``:
    the normalisation total the step's trace must carry in ``S``, to the last bit."""
    from neuralsteganography_amd.codec.errors import ArithmeticRangeError
    from neuralsteganography_amd.coder import RankDecodeSession, RankEncodeSession

    nb = len(expect)
    nsteps = _nsteps(expect)
    sess = RankEncodeSession(ctx, [e.payload for e in expect], temp=temp, quality=quality, max_tokens=nsteps + 4)
    sess.enable_trace()
    for t in range(nsteps):
        sess.trace.zero_()
        sess.step(step_rows(t))
        trace = _trace(sess)
        for s, e in enumerate(expect):
            got = trace[s]
            if t < len(e.steps):
                assert got == e.steps[t], f"{label} stream {s} step {t}: kernel {got} oracle {e.steps[t]}"
                if totals is not None:
                    assert float(sess.trace_rows().S[s]) == totals(s, t), f"{label} stream {s} step {t}: total"
            else:  # finished, or the step that found no capacity: nothing is emitted
                assert got == (0, 0, 0, 0, 0), f"{label} stream {s} step {t}: a step after the stream's last"
    assert _status(sess.fields()["flags"]) == [e.status for e in expect], f"{label}: per-stream status"
    toks, cons = _encoded(sess)
    assert toks == [e.tokens for e in expect], f"{label}: tokens differ from the oracle"
    assert cons == [e.consumed for e in expect] == sess.consumed(), f"{label}: consumption differs from the oracle"
    if vocab is not None:
        assert all(0 <= tok < vocab for tl in toks for tok in tl), f"{label}: a token outside the vocabulary"
    if any(e.status == "range" for e in expect):
        with pytest.raises(ArithmeticRangeError):
            sess.tokens()
    else:
        assert sess.all_done() and sess.tokens() == toks
    dec = RankDecodeSession(ctx, toks, cons, temp=temp, quality=quality)
    dec.enable_trace()
    assert dec.T == max(len(e.steps) for e in expect)
    for t in range(dec.T):
        dec.trace.zero_()
        dec.step(step_rows(t))
        trace = _trace(dec)
        for s, e in enumerate(expect):
            got = trace[s]
            want = e.steps[t] if t < len(e.steps) else (0, 0, 0, 0, 0)
            assert got == want, f"{label} decode stream {s} step {t}: kernel {got} oracle {want}"
            if totals is not None and t < len(e.steps):
                assert float(dec.trace_rows().S[s]) == totals(s, t), f"{label} decode stream {s} step {t}: total"
    out, status = _decoded(dec)
    assert status == ["open"] * nb and out == [e.decoded for e in expect], f"{label}: decoded payloads"
    assert dec.payloads() == out
    for s, e in enumerate(expect):
        if e.status == "done":
            assert out[s] == e.payload, f"{label} stream {s}: payload not recovered"


# ------------------------------------------------------------------------------------------------- logit rows
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_rank_coder_matches_oracle(case):
    expect = rv.expected(case)
    assert tuple(s for s, e in enumerate(expect) if e.status == "range") == case.err
    rows = _host_rows(lambda s, t: rv.case_row(case, s, t), B, _nsteps(expect))
    ctx = _ctx(case.vocab, case.dtype)
    for layout in LAYOUTS:
        _run_against_oracle(ctx, expect, _device_rows(rows, case.dtype, layout), temp=case.temp, quality=case.quality,
                            vocab=case.vocab, label=layout)


@pytest.mark.parametrize("vocab", [257, 131071])
def test_token_outside_the_first_2c_ranks_diverges_for_its_stream_only(vocab):
    """Stream 1's second token is replaced by the id of rank 2^c of that step (the first rank a payload cannot
    select; from numpy's order, confirmed by the oracle's own decode): NS_ST_ERR_DIVERGE for that stream, which keeps
    the bits of its first token; the other streams return their payloads."""
    from neuralsteganography_amd.codec.errors import DecodeDivergenceError
    from neuralsteganography_amd.coder import RankDecodeSession

    case = next(c for c in CASES if (c.vocab, c.dtype, c.policy, c.kind) == (vocab, "f32", "none", "synthetic"))
    expect = rv.expected(case)
    bad, at = 1, 1
    n, c, _, _, _ = expect[bad].steps[at]
    order, _, n_np = numpy_support(rv.case_row(case, bad, at), case.temp, {})
    assert n_np == n == vocab > 1 << c
    alien = int(order[1 << c])
    st = oracle.new_state(1)
    rc = oracle.rank_step_n(rv.case_row(case, bad, at), st, temp=case.temp, quality={}, token=alien, keep=c,
                            out_bits=np.zeros(16, np.uint8))[0]
    assert rc == oracle.OR_ERR_DIVERGE
    toks = [list(e.tokens) for e in expect]
    toks[bad][at] = alien
    rows = _host_rows(lambda s, t: rv.case_row(case, s, t), B, _nsteps(expect))
    for layout in LAYOUTS:
        fn = _device_rows(rows, case.dtype, layout)
        dec = RankDecodeSession(_ctx(vocab, "f32"), toks, [e.consumed for e in expect], temp=case.temp, quality={})
        for t in range(dec.T):
            dec.step(fn(t))
        out, status = _decoded(dec)
        assert status == ["diverge" if s == bad else "open" for s in range(B)], layout
        first = expect[bad].consumed[0] // 8
        assert out[bad] == expect[bad].payload[:first]
        assert [o for s, o in enumerate(out) if s != bad] == [e.payload for s, e in enumerate(expect) if s != bad]
        with pytest.raises(DecodeDivergenceError):
            dec.payloads()


# --------------------------------------------------------------------------------------------- ns_token_probs
PROBS_SEED, PROBS_TEMP, PROBS_B, PROBS_EXTRA, SENTINEL = 71, 0.8, 3, 37, -7.0


def _probs_policies(V):
    return [("none", {}), ("top_k", {"top_k": max(1, (2 * V) // 3)}), ("top_p", {"top_p": 0.9}),
            ("min_prob", {"min_prob": 0.5 / V}),
            ("combined", {"top_k": max(1, V // 2), "top_p": 0.95, "min_prob": 0.05 / V})]


@pytest.mark.parametrize("dtype", rv.DTYPES)
@pytest.mark.parametrize("vocab", [v for v, _ in rv.VOCABS])
def test_token_probs_match_the_reference_formula(vocab, dtype):
    """``ns_token_probs`` (next_token_probs, codec/distribution.py:107-142) on poisoned view rows, into an output
    wider than V pre-filled with a sentinel: the support is the oracle's n (V when nothing filters), the values are
    within 1e-12 absolute of the numpy float64 restatement, each row sums to 1, columns >= V are untouched."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _ptr, _stream_handle, rank_quality

    torch = _torch()
    npdt = np.float16 if dtype == "f16" else np.float32
    rows = _host_rows(lambda s, t: synthetic.logits_row(PROBS_SEED, s, t, vocab, 3.0, npdt), PROBS_B, 1)
    lg = _device_rows(rows, dtype, "view")(0)
    ctx = _ctx(vocab, dtype)
    stride = vocab + PROBS_EXTRA
    state = torch.zeros((PROBS_B, 4), dtype=torch.int64, device=lg.device)
    for name, q in _probs_policies(vocab):
        probs = torch.full((PROBS_B, stride), SENTINEL, dtype=torch.float64, device=lg.device)
        rq = rank_quality(q)
        rc = _lib.lib().ns_token_probs(ctx._h, _ptr(lg), lg.stride(0), PROBS_B, PROBS_TEMP, ctypes.byref(rq),
                                       _ptr(probs), stride, _ptr(state), _stream_handle())
        ctx.check(rc, "ns_token_probs")
        got = probs.cpu().numpy()
        assert np.all(got[:, vocab:] == SENTINEL), f"{name}: a column beyond V was written"
        for s in range(PROBS_B):
            order, ps, n_np = numpy_support(rows[0, s], PROBS_TEMP, q)
            n = rv.oracle_support(rows[0, s], PROBS_TEMP, q)
            assert n == n_np and (q or n == vocab)
            want = np.zeros(vocab)
            want[order[:n]] = ps[:n]
            want /= want.sum()
            assert int((got[s, :vocab] > 0).sum()) == n, f"{name} stream {s}: support"
            assert np.abs(got[s, :vocab] - want).max() < 1e-12, f"{name} stream {s}"
            assert abs(math.fsum(got[s, :vocab].tolist()) - 1.0) < 1e-12, f"{name} stream {s}: row sum"


# ---------------------------------------------------------------------------------------------- provider rows
@pytest.mark.parametrize("case", PROVIDER_CASES, ids=[c.id for c in PROVIDER_CASES])
def test_provider_rows_match_oracle(case):
    """float64 provider rows (ndarray by id, or dicts whose ids exceed 2^17) of different entry counts in one batch,
    staged as ``ProbRows`` for the rank sessions: tokens, history and n of ``or_rank_step64``; a row of one entry
    has no capacity (range error for that stream only)."""
    from neuralsteganography_amd.codec.distribution import ProbRows

    torch = _torch()
    expect = rv.provider_expected(case)
    ctx = _ctx(max(max(case.counts), 2), "f64", rv.PROVIDER_B)
    dev = torch.device("cuda", ctx.device)

    @functools.lru_cache(maxsize=None)
    def step_rows(t):
        rows = ProbRows([rv.provider_dist(case, s, t) for s in range(rv.PROVIDER_B)], dev, min_cols=ctx.params.vocab)
        assert rows.dict_rows == (case.form == "dict") and rows.count.tolist() == list(case.counts)
        return rows

    @functools.lru_cache(maxsize=None)
    def total(s, t):
        """apply_quality's renormalisation total (codec/quality.py:174-178) by numpy itself: ``sum()`` of the array
        with the n kept values at their positions and zeros elsewhere.  ``block_np_sum`` restates numpy's pairwise
        order, so the kernel's total (the trace's S) equals it bit for bit -- at every leaf shape the counts claim."""
        v = oracle.dist_arrays(rv.provider_dist(case, s, t))[0]
        order = np.lexsort((np.arange(v.size), -v))
        kept = np.zeros_like(v)
        kept[order[: expect[s].steps[t][0]]] = v[order[: expect[s].steps[t][0]]]
        assert float(kept.sum()) == oracle.np_sum(kept)
        return float(kept.sum())

    # (the crypto policy's total sums device log / exp values: tolerance-level, not compared)
    filtered = case.policy in ("topp", "minprob-topk")
    _run_against_oracle(ctx, expect, step_rows, temp=1.0, quality=case.quality, label=case.form,
                        totals=total if filtered else None)
    if case.form == "dict" and max(case.counts) > 64:
        assert any(tok >= 1 << 17 for e in expect for tok in e.tokens)


# ----------------------------------------------------------------------------------------------------- limits
def test_rank_context_beyond_17_bit_ids_is_refused():
    """The rank keys carry 17-bit ids: V = 131072 is the library's 'unsupported' error -- at context creation as
    ``HipRankLM`` sizes it (every id ranked), and at the first rank step or ``ns_token_probs`` call of a context whose
    own top-k is small -- and nothing is launched.  V = 131071 runs in ``test_rank_coder_matches_oracle``."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import CoderContext, CoderParams, RankEncodeSession, row_stride

    torch = _torch()
    V = rv.MAX_VOCAB + 1
    with pytest.raises(_lib.NativeLibraryError, match="supports vocab < 131072"):
        CoderContext(CoderParams(vocab=V, precision=16, temp=1.0, topk=V, dtype="f32", banned=[]), max_batch=2)
    ctx = CoderContext(CoderParams(vocab=V, precision=16, temp=1.0, topk=100, dtype="f32", banned=[]), max_batch=2)
    lg = torch.zeros((2, row_stride(V, "f32")), dtype=torch.float32, device="cuda")
    sess = RankEncodeSession(ctx, [b"ab", b"c"], temp=1.0, quality={})
    with pytest.raises(_lib.NativeLibraryError, match="rank coder: vocab must be < 131072"):
        sess.step(lg)
    assert sess.fields()["ntokens"].tolist() == [0, 0] and sess.fields()["bit_pos"].tolist() == [0, 0]
    assert any(c.vocab == rv.MAX_VOCAB for c in CASES)
