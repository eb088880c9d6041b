"""GPU: the rank steps with one quality row per stream (``ns_rank_encode_step_streams`` /
``ns_rank_decode_step_streams``) against the CPU oracle and against the scalar entries.

One session holds the 12 quality policies of ``tests/rank_vocab_cases.py`` at once: row r runs policy r (its
temperature included) on that case's stream ``s = r % 5``.  Bar: every step's (n, c, sel, take, token) is the oracle's
for that case and stream; the trace's S equals, bit for bit, what the scalar ``ns_rank_encode_step`` writes for that
stream alone with the case's (temp, quality); the row order changes nothing; the rows matter; a uniform table gives the
scalar entry's bytes; a finished stream is not touched; a bad table is refused before anything is launched.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from tests import rank_vocab_cases as rv

pytestmark = pytest.mark.gpu

VOCABS = (257, 4097, 8193)  # f32-tile-plus-1, chunk-plus-1, round-plus-1
SHAPES = [(v, d) for v in VOCABS for d in rv.DTYPES]
SENTINEL = -77


def _torch():
    import torch

    return torch


def _cases(vocab, dtype):
    out = [c for c in rv.CASES if c.kind == "synthetic" and c.vocab == vocab and c.dtype == dtype]
    assert len(out) == 12 and [c.policy for c in out] == [p[0] for p in rv.policies(vocab)]
    return out


@functools.lru_cache(maxsize=None)
def _ctx(vocab, dtype, max_batch=12):
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    return CoderContext(CoderParams(vocab=vocab, precision=16, temp=1.0, topk=vocab, dtype=dtype, banned=[]),
                        max_batch=max_batch)


def _expected(case, r):
    e = rv.expected(case)[r % rv.B]
    assert e.status == "done" and 2 <= len(e.steps) <= 15
    return e


@functools.lru_cache(maxsize=None)
def _logits(vocab, dtype):
    """[nsteps, 12, ld] on the device: row r of step t is ``case_row(case_r, r % 5, t)``; the pad columns hold NaN."""
    from neuralsteganography_amd.coder import row_stride

    cases = _cases(vocab, dtype)
    nsteps = max(len(_expected(c, r).steps) for r, c in enumerate(cases))
    host = np.full((nsteps, 12, row_stride(vocab, dtype)), np.nan, cases[0].npdt)
    for t in range(nsteps):
        for r, c in enumerate(cases):
            host[t, r, :vocab] = rv.case_row(c, r % rv.B, t)
    return _torch().from_numpy(host).cuda()


def _table(cases):
    from neuralsteganography_amd.coder import RankStreamQuality

    return RankStreamQuality.from_qualities([c.quality for c in cases], [c.temp for c in cases])


def _encode(vocab, dtype, order, qrows=None):
    """The 12 rows in session order ``order`` (session row i holds table row order[i]); per TABLE row: the steps'
    (n, c, sel, take, token), their S bit patterns, tokens and consumption."""
    from neuralsteganography_amd.coder import RankStreamEncodeSession

    torch = _torch()
    cases = _cases(vocab, dtype)
    lg = _logits(vocab, dtype)
    idx = torch.as_tensor(np.asarray(order), device=lg.device)
    q = (qrows if qrows is not None else _table(cases)).take(order)
    sess = RankStreamEncodeSession(_ctx(vocab, dtype), 12, payloads=[rv.payload(r % rv.B) for r in order], quality=q)
    sess.enable_trace()
    steps = [[] for _ in range(12)]
    totals = [[] for _ in range(12)]
    for t in range(lg.shape[0]):
        live = (sess.fields()["flags"] & 1) == 0
        sess.trace.zero_()
        sess.step(lg[t].index_select(0, idx).contiguous())
        tr = sess.trace_rows()
        for i, r in enumerate(order):
            got = (int(tr.k[i]), int(tr.kprime[i]), int(tr.sel[i]), int(tr.n[i]), int(tr.token[i]))
            if live[i] and got != (0, 0, 0, 0, 0):
                steps[r].append(got)
                totals[r].append(np.float64(tr.S[i]).view(np.uint64))
            else:
                assert got == (0, 0, 0, 0, 0), f"row {r} step {t}: a finished stream wrote a trace"
    assert sess.all_done()
    toks, cons = sess.tokens(), sess.consumed()
    back = {r: i for i, r in enumerate(order)}
    return steps, totals, [toks[back[r]] for r in range(12)], [cons[back[r]] for r in range(12)]


@functools.lru_cache(maxsize=None)
def _mixed(vocab, dtype):
    return _encode(vocab, dtype, list(range(12)))


@functools.lru_cache(maxsize=None)
def _scalar_totals(vocab, dtype):
    """Per table row: the S of every step of the scalar ``ns_rank_encode_step`` for that stream alone (B = 1)."""
    from neuralsteganography_amd.coder import RankEncodeSession

    lg = _logits(vocab, dtype)
    out = []
    for r, c in enumerate(_cases(vocab, dtype)):
        sess = RankEncodeSession(_ctx(vocab, dtype), [rv.payload(r % rv.B)], temp=c.temp, quality=c.quality)
        sess.enable_trace()
        tot = []
        for t in range(len(_expected(c, r).steps)):
            sess.step(lg[t, r:r + 1])
            tot.append(np.float64(sess.trace_rows().S[0]).view(np.uint64))
        assert sess.all_done() and sess.tokens()[0] == _expected(c, r).tokens
        out.append(tot)
    return out


@pytest.mark.parametrize("vocab,dtype", SHAPES)
def test_every_row_runs_its_own_policy_as_the_oracle_does(vocab, dtype):
    steps, _, toks, cons = _mixed(vocab, dtype)
    for r, c in enumerate(_cases(vocab, dtype)):
        e = _expected(c, r)
        assert steps[r] == list(e.steps), f"row {r} ({c.policy}): steps differ from the oracle"
        assert toks[r] == e.tokens and cons[r] == e.consumed, f"row {r} ({c.policy})"


@pytest.mark.parametrize("vocab,dtype", SHAPES)
def test_decode_streams_returns_the_payloads(vocab, dtype):
    from neuralsteganography_amd.coder import RankStreamDecodeSession

    cases = _cases(vocab, dtype)
    _, _, toks, cons = _mixed(vocab, dtype)
    lg = _logits(vocab, dtype)
    dec = RankStreamDecodeSession(_ctx(vocab, dtype), 12, max_tokens=max(map(len, toks)), max_bits=8 * 8,
                                  token_lists=toks, histories=cons, quality=_table(cases))
    dec.enable_trace()
    for t in range(lg.shape[0]):
        dec.trace.zero_()
        dec.step(lg[t])
        tr = dec.trace_rows()
        for r, c in enumerate(cases):
            e = _expected(c, r)
            got = (int(tr.k[r]), int(tr.kprime[r]), int(tr.sel[r]), int(tr.n[r]), int(tr.token[r]))
            assert got == (e.steps[t] if t < len(e.steps) else (0, 0, 0, 0, 0)), f"row {r} decode step {t}"
    assert dec.payloads() == [rv.payload(r % rv.B) for r in range(12)]


@pytest.mark.parametrize("vocab,dtype", SHAPES)
def test_trace_total_equals_the_scalar_entry_bit_for_bit(vocab, dtype):
    _, totals, _, _ = _mixed(vocab, dtype)
    want = _scalar_totals(vocab, dtype)
    for r, c in enumerate(_cases(vocab, dtype)):
        assert totals[r] == want[r], f"row {r} ({c.policy}, temp {c.temp}): S differs from the scalar entry"


@pytest.mark.parametrize("vocab,dtype", SHAPES)
def test_row_order_changes_nothing(vocab, dtype):
    steps, totals, toks, cons = _mixed(vocab, dtype)
    rsteps, rtotals, rtoks, rcons = _encode(vocab, dtype, list(range(11, -1, -1)))
    assert (rsteps, rtotals, rtoks, rcons) == (steps, totals, toks, cons)


@pytest.mark.parametrize("vocab,dtype", SHAPES)
def test_the_rows_matter(vocab, dtype):
    """Row 0's values (policy ``none``, temperature 1) in every row: at least 5 of the other 11 streams give other
    tokens (the oracle gives other tokens than policy ``none`` for 7 of every 12)."""
    cases = _cases(vocab, dtype)
    _, _, toks, _ = _mixed(vocab, dtype)
    _, _, same, _ = _encode(vocab, dtype, list(range(12)), qrows=_table([cases[0]] * 12))
    assert same[0] == toks[0]
    assert sum(same[r] != toks[r] for r in range(1, 12)) >= 5


@pytest.mark.parametrize("dtype", rv.DTYPES)
@pytest.mark.parametrize("policy", ["cap3", "ptemp0.7"])
def test_uniform_table_gives_the_scalar_entrys_bytes(policy, dtype):
    """B = 5, one policy in every row, V = 4097: tokens, history, states and every step's trace as bytes."""
    from neuralsteganography_amd.coder import RankEncodeSession, RankStreamEncodeSession, row_stride

    torch = _torch()
    V = 4097
    case = next(c for c in _cases(V, dtype) if c.policy == policy)
    assert ("cap_per_token_bits" in case.quality) or ("prob_temp" in case.quality)
    expect = rv.expected(case)
    nsteps = max(len(e.steps) for e in expect)
    host = np.full((nsteps, rv.B, row_stride(V, dtype)), np.nan, case.npdt)
    for t in range(nsteps):
        for s in range(rv.B):
            host[t, s, :V] = rv.case_row(case, s, t)
    lg = torch.from_numpy(host).cuda()
    pls = [rv.payload(s) for s in range(rv.B)]
    ctx = _ctx(V, dtype)
    a = RankEncodeSession(ctx, pls, temp=case.temp, quality=case.quality, max_tokens=128)
    b = RankStreamEncodeSession(ctx, rv.B, payloads=pls, quality=_table([case] * rv.B), max_tokens=128)
    a.enable_trace(), b.enable_trace()
    for t in range(nsteps):
        a.step(lg[t]), b.step(lg[t])
        assert a.trace.cpu().numpy().tobytes() == b.trace.cpu().numpy().tobytes(), f"trace of step {t}"
        assert a.out_token.cpu().numpy().tobytes() == b.out_token.cpu().numpy().tobytes()
    assert a.all_done() and a.tokens() == [e.tokens for e in expect]
    assert a.hist.shape == b.hist.shape
    for name in ("state", "hist", "cons"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name


def test_a_finished_stream_is_not_touched():
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import RankStreamEncodeSession

    vocab, dtype = 257, "f32"
    cases = _cases(vocab, dtype)
    lg = _logits(vocab, dtype)
    sess = RankStreamEncodeSession(_ctx(vocab, dtype), 12, payloads=[rv.payload(r % rv.B) for r in range(12)],
                                   quality=_table(cases))
    sess.enable_trace()
    lens = [len(_expected(c, r).steps) for r, c in enumerate(cases)]
    first = int(np.argmin(lens))
    assert lens[first] + 2 <= lg.shape[0], "the shortest stream ends two steps before the longest"
    for t in range(lens[first]):
        sess.step(lg[t])
    f = sess.fields()
    assert f["flags"][first] & _lib.NS_ST_DONE and not (f["flags"] & _lib.NS_ST_DONE).all()
    n = int(f["ntokens"][first])
    sess.out_token[first] = SENTINEL
    sess.hist[first, n:] = SENTINEL
    sess.cons[first, n:] = SENTINEL
    sess.trace[first] = SENTINEL
    state = sess.state[first].clone()
    for t in range(lens[first], lens[first] + 2):
        sess.step(lg[t])
    assert int(sess.out_token[first]) == SENTINEL
    assert (sess.hist[first, n:] == SENTINEL).all() and (sess.cons[first, n:] == SENTINEL).all()
    assert (sess.trace[first] == SENTINEL).all()
    assert _torch().equal(sess.state[first], state)
    assert (sess.fields()["ntokens"] > f["ntokens"]).any(), "the live streams went on"


def test_bad_tables_are_refused_and_nothing_is_launched():
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import (CoderContext, CoderParams, RankStreamDecodeSession,
                                               RankStreamEncodeSession, StreamQuality, _ptr, _stream_handle)

    torch = _torch()
    vocab, dtype = 257, "f32"
    cases = _cases(vocab, dtype)
    ctx = _ctx(vocab, dtype)
    lg = _logits(vocab, dtype)[0].contiguous()
    sess = RankStreamEncodeSession(ctx, 12, payloads=[rv.payload(r % rv.B) for r in range(12)], quality=_table(cases))
    dec = RankStreamDecodeSession(ctx, 12, max_tokens=4, max_bits=64, token_lists=[[1, 2]] * 12,
                                  histories=[[1, 1]] * 12, quality=_table(cases))
    L = _lib.lib()

    def enc(c, table):
        return L.ns_rank_encode_step_streams(c._h, _ptr(lg), lg.stride(0), 12, _ptr(sess.payload),
                                             sess.payload.stride(0), _ptr(sess.nbits), _ptr(sess.state),
                                             _ptr(sess.out_token), _ptr(sess.hist), _ptr(sess.cons),
                                             sess.hist.shape[1], table, None, 0, _stream_handle())

    def dcd(c, table):
        tok = torch.ones(12, dtype=torch.int32, device=lg.device)
        act = torch.ones(12, dtype=torch.uint8, device=lg.device)
        return L.ns_rank_decode_step_streams(c._h, _ptr(lg), lg.stride(0), 12, _ptr(tok), _ptr(tok), _ptr(act),
                                             _ptr(dec.state), _ptr(dec.out_bits), dec.out_stride, table, None, 0,
                                             _stream_handle())

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (sess.state, sess.out_token, sess.hist, dec.state, dec.out_bits)]

    before = snapshot()
    good = sess.qtable.data_ptr()
    assert good % 8 == 0
    for call in (enc, dcd):
        assert call(ctx, None) == _lib.NS_ERR_CONFIG                      # null table
        assert call(ctx, ctypes.c_void_p(good + 4)) == _lib.NS_ERR_CONFIG  # odd address
        assert call(ctx, ctypes.c_void_p(good + 1)) == _lib.NS_ERR_CONFIG
    # a registered ns_set_stream_quality table: the rank steps refuse to run beside it
    small = StreamQuality([CoderParams(vocab=vocab, precision=16, temp=1.0, topk=8, dtype=dtype, banned=[])] * 12)
    reg = small.table(lg.device)
    assert L.ns_set_stream_quality(ctx._h, _ptr(reg), small.k_max) == _lib.NS_OK
    try:
        for call in (enc, dcd):
            assert call(ctx, ctypes.c_void_p(good)) == _lib.NS_ERR_CONFIG
    finally:
        assert L.ns_set_stream_quality(ctx._h, None, 0) == _lib.NS_OK
    # provider probability rows stay on the scalar entries
    c64 = CoderContext(CoderParams(vocab=vocab, precision=16, temp=1.0, topk=vocab, dtype="f64", banned=[]),
                       max_batch=12)
    for call in (enc, dcd):
        assert call(c64, ctypes.c_void_p(good)) == _lib.NS_ERR_CONFIG
    assert snapshot() == before
    # and the same call with the good table runs
    assert enc(ctx, ctypes.c_void_p(good)) == _lib.NS_OK
    assert (sess.fields()["ntokens"] == 1).all()
