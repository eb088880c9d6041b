"""GPU: the per-stream sampler step (``ns_sample_step_streams``) through ``SampleSession`` on synthetic rows, B = 8,
12 steps: every stream with its own temperature, top-k, length, seed and draw id against the oracle run with that
stream's own values (``tests/sample_stream_cases.py``; the host file shows that the cases discriminate).  Tokens are
bit-exact; statistics within rel 1e-4 (fp32 rows) / 1e-3 (fp16 rows), the tolerances of
``tests/test_gpu_sampler_stats.py``."""

from __future__ import annotations

import numpy as np
import pytest

from neuralsteganography_amd import _lib
from neuralsteganography_amd.exceptions import ConfigurationError
from oracle import oracle
from tests import sample_stream_cases as sc

pytestmark = pytest.mark.gpu


def _quality(case, order):
    from neuralsteganography_amd.coder import CoderParams, StreamQuality

    return StreamQuality([CoderParams(vocab=case.vocab, precision=16, temp=case.streams[s].temp, topk=case.topk_of(s),
                                      dtype=case.dtype) for s in order], k_max=case.k_max_row)


def _session(case, order, trace=False, max_tokens=sc.MAX_STEPS):
    from neuralsteganography_amd.coder import CoderContext, SampleSession

    sq = _quality(case, order)
    ctx = CoderContext(sq.context_params(), max_batch=len(order))
    st = [case.streams[s] for s in order]
    sess = SampleSession(ctx, len(order), max_tokens=max_tokens, stats=True, quality=sq, seeds=[q.seed for q in st],
                         gids=[q.gid for q in st], lengths=[q.length for q in st])
    if trace:
        sess.enable_trace()
    return sess


def _run(case, order, steps=sc.MAX_STEPS, sess=None, first=0):
    import torch

    from neuralsteganography_amd.coder import row_stride

    sess = sess if sess is not None else _session(case, order)
    ld = row_stride(case.vocab, case.dtype) + case.pad
    for t in range(first, first + steps):
        sess.step(torch.from_numpy(sc.logits_batch(case, order, t, ld)).cuda())
    return sess


@pytest.mark.parametrize("name", list(sc.NAMES))
def test_every_stream_matches_the_oracle_of_its_own_row(name):
    case = sc.case(name)
    order = list(range(len(case.streams)))
    sess = _run(case, order)
    toks, stats = sess.tokens(), sess.stats()
    rel = 1e-3 if case.dtype == "f16" else 1e-4
    for s, (ref, acc) in enumerate(sc.reference(name)):
        assert toks[s] == ref, f"{name} stream {s}: sampled tokens differ from the oracle"
        want = oracle.stats_summary(acc)
        for k in ("avg_NLL", "avg_KL", "avg_Hq"):
            assert stats[s][k] == pytest.approx(want[k], rel=rel, abs=rel / 10), (name, s, k)


@pytest.mark.parametrize("name", ["single_f16", "wide_f32"])
def test_a_stream_keeps_its_tokens_in_any_row(name):
    """The property slots rest on: the same streams in a permuted row order, and one stream alone in row 0 of a
    B = 1 launch, get the tokens they get in their own row."""
    case = sc.case(name)
    ref = sc.reference(name)
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    toks = _run(case, order).tokens()
    for row, s in enumerate(order):
        assert toks[row] == ref[s][0], (name, row, s)
    for s in (2, 5):  # topk 1 / the limit (single-pass), every id (wide)
        assert _run(case, [s]).tokens() == [ref[s][0]], (name, s)


@pytest.mark.parametrize("name", ["single_f32", "wide_f32"])
def test_parked_streams_are_not_written(name):
    """Past its length a stream's state, history row, statistics row, trace row and out_token are bit-identical
    before and after further steps, and its history holds exactly ``length`` tokens."""
    case = sc.case(name)
    order = list(range(len(case.streams)))
    lens = np.asarray([q.length for q in case.streams])
    sess = _session(case, order, trace=True, max_tokens=sc.MAX_STEPS + 2)
    _run(case, order, steps=5, sess=sess)  # the streams of length 1 and 5 are parked now

    def snap():
        return [getattr(sess, k).cpu().numpy().copy() for k in ("state", "hist", "stats_acc", "trace", "out_token")]

    before = snap()
    _run(case, order, steps=sc.MAX_STEPS - 5 + 2, sess=sess, first=5)  # two steps past the longest length as well
    after = snap()
    parked = np.nonzero(lens <= 5)[0]
    assert parked.size == 3
    for a, b in zip(before, after):
        assert a[parked].tobytes() == b[parked].tobytes()
    hist = after[1]
    ref = sc.reference(name)
    for s in order:
        assert hist[s, : lens[s]].tolist() == ref[s][0]
        assert (hist[s, lens[s]:] == -1).all()
    f = sess.state.cpu().numpy().view(np.int32).reshape(len(order), 8)
    assert f[:, 6].tolist() == lens.tolist()  # ntokens stops at the length
    assert after[2][:, 3].tolist() == lens.astype(float).tolist()  # as many counted steps


def test_refusals_and_the_registered_table_rule():
    import torch

    from neuralsteganography_amd.coder import CoderContext, CoderParams, SampleSession, row_stride, sample_draw_rows

    case = sc.case("single_f32")
    B = len(case.streams)
    order = list(range(B))
    sess = _session(case, order)
    ctx, L = sess.ctx, _lib.lib()
    ld = row_stride(case.vocab, case.dtype)
    rows = torch.from_numpy(sc.logits_batch(case, order, 0, ld)).cuda()
    ban = (ctx._banned, ctx._nbanned)

    def call(c=ctx, q=sess.qtable.data_ptr(), d=sess.draws.data_ptr(), k=sess.k_max, lg=rows):
        return L.ns_sample_step_streams(c._h, lg.data_ptr(), lg.stride(0), B, q, d, k, sess.state.data_ptr(),
                                        sess.out_token.data_ptr(), sess.hist.data_ptr(), sess.hist.shape[1], *ban,
                                        None, None, 0, None)

    state0 = sess.state.cpu().numpy().copy()
    assert call(q=None) == _lib.NS_ERR_CONFIG  # a null table
    assert call(d=None) == _lib.NS_ERR_CONFIG
    assert call(q=sess.qtable.data_ptr() + 4) == _lib.NS_ERR_CONFIG  # a misaligned table
    assert call(d=sess.draws.data_ptr() + 4) == _lib.NS_ERR_CONFIG
    assert call(k=0) == _lib.NS_ERR_CONFIG  # k_max < 1
    f64 = CoderContext(CoderParams(vocab=case.vocab, dtype="f64"), max_batch=B)
    assert call(c=f64) == _lib.NS_ERR_CONFIG  # an F64 context
    # a k_max on the wide path needs a context created for it, worded as the encode entries word it
    assert call(k=sc.limit("f32") + 1) == _lib.NS_ERR_CONFIG
    assert "create the context with max_k >= topk" in L.ns_last_error(ctx._h).decode()
    torch.cuda.synchronize()
    assert sess.state.cpu().numpy().tobytes() == state0.tobytes()  # a refused call launched nothing

    # a registered quality table: both sampler entries refuse, as ns_sample_step always has
    plain = SampleSession(ctx, B, seed=1, topk=40, temp=1.0, max_tokens=2, stats=False)
    assert L.ns_set_stream_quality(ctx._h, sess.qtable.data_ptr(), sess.k_max) == _lib.NS_OK
    try:
        assert call() == _lib.NS_ERR_CONFIG
        with pytest.raises(ConfigurationError):
            plain.step(rows)
        with pytest.raises(ConfigurationError):
            sess.step(rows)
    finally:
        L.ns_set_stream_quality(ctx._h, None, 0)
    # ... and without one the new entry runs (the old one too)
    sess.step(rows)
    plain.step(rows)
    ref = sc.reference("single_f32")
    assert [t[0] for t in sess.tokens()] == [r[0][0] for r in ref]
    # the session refuses tables that do not fit it
    with pytest.raises(ConfigurationError):
        SampleSession(ctx, B, quality=_quality(case, order))  # rows without seeds, gids and lengths
    with pytest.raises(ConfigurationError):
        SampleSession(ctx, B, seeds=[1] * B, gids=[0] * B, lengths=[1] * B)  # ... and the other way round
    with pytest.raises(ConfigurationError):
        SampleSession(ctx, B, quality=_quality(case, order), seeds=[1], gids=[0], lengths=[1])
    assert sample_draw_rows([1], [2], [3]).tolist() == [[1, 2, 3, 0]]
