"""GPU: one coder quality (temperature, top-k, precision) per message in one batch (``ns_set_stream_quality``,
``encode_batch(qualities=...)``, ``stego_encode_batch(qualities=...)``; the reference's unit of work is one message
with its own ``quality``, ``code_base/arithmetic.py:78-88``).

The contract: a stream's tokens, bits and step traces are those of a call with that stream's quality alone.  Every
comparison is exact (token lists, bit lists, trace integers) against the CPU oracle run with the stream's own
(temp, precision, topk), or against the existing one-quality path; the statistics keep the project's bound
(rel 2e-5, abs 2e-6, as ``tests/test_gpu_sampler_stats.py``).  Each reference fixture also checks that at least 5 of
its 7 streams come out differently under the batch's FIRST quality, so a step that applied one quality to every
stream could not pass.
"""

import ctypes
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

# ------------------------------------------------------------------------------------------------------ kernel
V, B, SEED, SCALE, NSTEP = 50257, 7, 31, 3.0, 24  # B = 7: two workgroups of the wave-per-stream form, one partial
NBYTES = 64  # payload per stream: more than any quality consumes in 24 steps (at most about 200 bits)


def _qualities(dtype):
    """(topk, temp, precision) per stream: every rank-slot bucket edge (<= 128, <= 320, beyond) up to the dtype's
    single-pass limit in one launch, four temperatures, four precisions; stream 4's 1/R cutoff binds (R <= 2^12)."""
    limit = _lib.max_topk(_lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32)
    return [(2, 0.7, 12), (40, 0.9, 16), (128, 1.0, 26), (129, 1.3, 40), (320, 0.7, 12), (321, 0.9, 26),
            (limit, 1.0, 40)]


def _params(dtype, q):
    return CoderParams(vocab=V, precision=q[2], temp=q[1], topk=q[0], dtype=dtype)


def _oracle(dtype, s, bits, q, stats=None):
    """NSTEP oracle encode steps of stream s under quality q: tokens, (k, k', sel, n, token) traces, final bit_pos."""
    npdt = np.float16 if dtype == "f16" else np.float32
    packed = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    st = oracle.new_state(q[2])
    toks, traces = [], []
    for t in range(NSTEP):
        row = synthetic.logits_row(SEED, s, t, V, SCALE, npdt).astype(np.float32)
        rc, tok, tr = oracle.encode_step(row, st, packed, len(bits), banned=[V - 1, 628], temp=q[1], precision=q[2],
                                         topk=q[0], stats=stats)
        assert rc == 0 and st.bit_pos < len(bits)
        toks.append(tok)
        traces.append((tr.k, tr.kprime, tr.sel, tr.n, tr.token))
    return toks, traces, int(st.bit_pos)


@functools.lru_cache(maxsize=None)
def _reference(dtype):
    """Per dtype, computed once on the CPU: the payloads and the oracle's tokens and traces of every stream under
    its OWN quality -- and the check that the batch's first quality would give other tokens."""
    qs = _qualities(dtype)
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(900 + s, NBYTES)) for s in range(B)]
    expect = [_oracle(dtype, s, bits[s], qs[s]) for s in range(B)]
    assert any(tr[0] < q[0] for e, q in zip(expect, qs) for tr in e[1]), "no step whose 1/R cutoff binds"
    under_first = [_oracle(dtype, s, bits[s], qs[0])[0] for s in range(B)]
    assert sum(a != e[0] for a, e in zip(under_first, expect)) >= 5, "the batch's first quality gives the same tokens"
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
    return dtype, qs, bits, expect, rows, sq


@pytest.fixture(params=["f32", "f16"])
def case(request):
    return _case(request.param)


@pytest.fixture(params=["wave", "auto"])
def form(request):
    """The wave-per-stream form, and the automatic choice (at B = 7 the split form: one workgroup per stream)."""
    prev = _lib.set_split_max_batch(0 if request.param == "wave" else -1)
    yield request.param
    _lib.set_split_max_batch(prev)


def _run_encode(ctx, bits, rows, sq, expect=None, **step_kw):
    sess = EncodeSession(ctx, bits, quality=sq, stats=step_kw.pop("stats", False))
    sess.enable_trace()
    for t in range(NSTEP):
        sess.step(rows[t], **step_kw)
        if expect is not None:
            tr = sess.trace_rows()
            for s in range(len(bits)):
                if t < len(expect[s][1]):
                    got = (int(tr.k[s]), int(tr.kprime[s]), int(tr.sel[s]), int(tr.n[s]), int(tr.token[s]))
                    assert got == expect[s][1][t], f"stream {s} step {t}: kernel {got} oracle {expect[s][1][t]}"
    assert not (sess.fields()["flags"] & (_lib.NS_ST_DONE | _lib.NS_ST_ERR_RANGE)).any()
    assert sess.fields()["bit_pos"].tolist() == [e[2] for e in expect]
    return sess


def test_mixed_rows_match_the_oracle_of_each_streams_own_quality(case, form):
    dtype, qs, bits, expect, rows, sq = case
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _run_encode(ctx, bits, rows, sq, expect)
    toks = sess.tokens()
    assert toks == [e[0] for e in expect]
    hi = sess.fields()["hi"]
    assert all(int(hi[s]) <= 1 << qs[s][2] for s in range(B))
    dec = DecodeSession(ctx, toks, quality=sq)
    assert dec.out_stride >= (dec.T * 40 + 40 + 7) // 8  # sized for the call's largest precision
    for t in range(dec.T):
        dec.step(rows[t])
    out = dec.bits()
    for s in range(B):
        # every token but the last gives back the n payload bits it fixed; the last one emits all `precision` bits
        # of the interval's bottom (code_base/arithmetic.py:356-357) -- the precision of this stream's row
        fixed = sum(tr[3] for tr in expect[s][1][:-1])
        assert fixed >= 8 and len(out[s]) == fixed + qs[s][2], s
        assert out[s][:fixed] == bits[s][:fixed], f"stream {s}: decoded bits differ from the payload"


def test_init_state_takes_each_rows_precision(case):
    dtype, qs, bits, _, _, sq = case
    ctx = CoderContext(sq.context_params(), max_batch=B)
    f = EncodeSession(ctx, bits, quality=sq).fields()
    assert f["hi"].tolist() == [1 << q[2] for q in qs] and not f["lo"].any() and not f["bit_pos"].any()
    assert EncodeSession(ctx, bits).fields()["hi"].tolist() == [1 << 40] * B  # no table: the context's precision


def test_statistics_build_with_a_table():
    dtype, qs, bits, expect, rows, sq = _case("f16")  # one statistics case: fp16 rows, automatic (split) form
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _run_encode(ctx, bits, rows, sq, expect, stats=True)
    assert sess.tokens() == [e[0] for e in expect]
    got = sess.stats()
    for s in range(B):
        acc = np.zeros(4)
        _oracle(dtype, s, bits[s], qs[s], stats=acc)
        want = oracle.stats_summary(acc, expect[s][2])
        for k, v in want.items():
            assert got[s][k] == pytest.approx(v, rel=2e-5, abs=2e-6), (s, k)


def test_forced_exact_sum_with_a_table():
    dtype, qs, bits, expect, rows, sq = _case("f32")  # one forced-exact case: fp32 rows, wave-per-stream form
    prev = _lib.set_split_max_batch(0)
    try:
        ctx = CoderContext(sq.context_params(), max_batch=B)
        sess = _run_encode(ctx, bits, rows, sq, expect, force_exact=True)
    finally:
        _lib.set_split_max_batch(prev)
    assert sess.tokens() == [e[0] for e in expect]
    assert ctx.counters()[0] >= B * NSTEP  # every stream-step took the exact-sum path


def test_equal_rows_give_the_scalar_calls_outputs(case, form):
    dtype, _, bits, _, rows, _ = case
    p = CoderParams(vocab=V, precision=26, temp=0.9, topk=300, dtype=dtype)
    ctx = CoderContext(p, max_batch=B)
    outs = []
    for sq in (None, StreamQuality([p] * B)):
        sess = EncodeSession(ctx, bits, quality=sq)
        sess.enable_trace()
        traces = []
        for t in range(NSTEP):
            sess.step(rows[t])
            traces.append(sess.trace.cpu().numpy().copy())
        dec = DecodeSession(ctx, sess.tokens(), quality=sq)
        for t in range(dec.T):
            dec.step(rows[t])
        outs.append((sess.tokens(), np.stack(traces), sess.state.cpu().numpy(), dec.bits()))
    assert outs[0][0] == outs[1][0] and outs[0][3] == outs[1][3]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_table_is_refused_where_it_does_not_apply(case):
    dtype, qs, bits, _, rows, sq = case
    L = _lib.lib()
    limit = _lib.max_topk(_lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32)
    table = sq.table(torch.device("cuda", 0))
    wide = CoderContext(CoderParams(vocab=V, precision=26, topk=limit + 1, dtype=dtype), max_batch=B)
    assert L.ns_set_stream_quality(wide._h, table.data_ptr(), limit + 1) == _lib.NS_ERR_UNSUPPORTED
    ctx = CoderContext(sq.context_params(), max_batch=B)
    assert L.ns_set_stream_quality(ctx._h, table.data_ptr(), 0) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality(ctx._h, table.data_ptr() + 4, limit) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality(None, table.data_ptr(), limit) == _lib.NS_ERR_CONFIG
    smp = SampleSession(ctx, B, seed=1, topk=40, temp=1.0, max_tokens=2, stats=False)
    assert L.ns_set_stream_quality(ctx._h, table.data_ptr(), limit) == _lib.NS_OK
    try:
        with pytest.raises(ConfigurationError):
            smp.step(rows[0])
        q = _lib.NsRankQuality(0, 0, 0.0, -1.0, 0.0)
        probs = torch.zeros((B, V), dtype=torch.float64, device="cuda")
        rc = L.ns_token_probs(ctx._h, rows[0].data_ptr(), rows[0].stride(0), B, 1.0, ctypes.byref(q),
                              probs.data_ptr(), V, smp.state.data_ptr(), None)
        assert rc == _lib.NS_ERR_CONFIG
    finally:
        assert L.ns_set_stream_quality(ctx._h, None, 0) == _lib.NS_OK
    smp.step(rows[0])  # cleared: the sampler runs again
    torch.cuda.synchronize()
    with pytest.raises(ConfigurationError):
        EncodeSession(ctx, bits[:3], quality=sq)  # one row per stream
    with pytest.raises(ConfigurationError):
        EncodeSession(CoderContext(_params(dtype, qs[1]), max_batch=B), bits, quality=sq)  # context below k_max


# ---------------------------------------------------------------------------------------------------- provider
# the tiny model of tests/test_gpu_context_batch.py: vocab 512, so no speculative sample (spec_j = 0 rows)
QS = [{"temp": 0.9, "precision": 26, "topk": 300}, {"temp": 0.7, "precision": 16, "topk": 40},
      {"temp": 1.3, "precision": 12, "topk": 128}, {"temp": 1.0, "precision": 40, "topk": 500},
      {"temp": 0.9, "precision": 26, "topk": 2}]
Q_OF = [0, 1, 2, 3, 4, 1, 3]  # 7 messages, 5 distinct qualities
CTX_LENS = [1, 31, 32, 33, 64, 65, 100]


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


def _provider(**kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(n_bytes, seed0=500):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _contexts(seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 511, size=n).tolist() for n in CTX_LENS]


@pytest.fixture(scope="module")
def provider_reference():
    """Every message alone with its own quality (the existing one-quality path), computed once."""
    lm = _provider()
    context = _contexts()[3]
    bits = _bits([4, 12, 7, 9, 5, 11, 8])
    qs = [QS[i] for i in Q_OF]
    ref = [lm.encode_batch([b], context, quality=q)[0] for b, q in zip(bits, qs)]
    under_first = lm.encode_batch(bits, context, quality=qs[0])
    assert sum(a != b for a, b in zip(under_first, ref)) >= 5, "the first quality gives the same tokens"
    return lm, context, bits, qs, ref


@pytest.mark.parametrize("mode", ["graphs", "eager", "small_budget"])
def test_encode_and_decode_batch_with_qualities_equal_each_message_alone(provider_reference, mode):
    lm, context, bits, qs, ref = provider_reference
    kw = dict(graphs=mode != "eager")
    lm.slot_budget_tokens = 8 if mode == "small_budget" else None  # table growth and graph re-capture
    try:
        got = lm.encode_batch(bits, context, qualities=qs, slots=3, **kw)  # 7 messages, 3 slots: refills
        sched = dict(lm.last_schedule)
        out = lm.decode_batch(got, context, qualities=qs, slots=3, **kw)
        dsched = dict(lm.last_decode_schedule)
    finally:
        lm.slot_budget_tokens = None
    assert got == ref
    assert sched["quality_groups"] == 1 and dsched["quality_groups"] == 1 and sched["slots"] == 3
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    if mode == "graphs":  # the receiver's side: each message alone with its own quality
        for m in range(len(bits)):
            alone = lm.decode_batch([got[m]], context, quality=qs[m])[0]
            assert alone[: len(bits[m])] == bits[m], m


def test_qualities_compose_with_contexts_and_statistics(provider_reference):
    lm, _, bits, qs, _ = provider_reference
    ctxs = _contexts()
    ref = [lm.encode_batch([b], c, quality=q, return_stats=True) for b, c, q in zip(bits, ctxs, qs)]
    got, stats = lm.encode_batch(bits, contexts=ctxs, qualities=qs, slots=3, return_stats=True)
    assert got == [r[0][0] for r in ref]
    assert lm.last_schedule["prefill_rows"] == sum(CTX_LENS)
    for m, r in enumerate(ref):
        for k, v in r[1][0].items():
            assert stats[m][k] == pytest.approx(v, rel=2e-5, abs=2e-6), (m, k)
    out = lm.decode_batch(got, contexts=ctxs, qualities=qs, slots=3)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


def test_compaction_permutes_the_table(provider_reference):
    lm, context, _, qs, _ = provider_reference
    bits = _bits([3, 3, 40, 3, 3, 3, 36], seed0=640)  # two long messages outlive the others: 7 slots -> 2
    ref = [lm.encode_batch([b], context, quality=q)[0] for b, q in zip(bits, qs)]
    got = lm.encode_batch(bits, context, qualities=qs)
    assert lm.last_schedule["compactions"] > 0, lm.last_schedule
    assert got == ref
    out = lm.decode_batch(got, context, qualities=qs)
    assert lm.last_decode_schedule["compactions"] > 0, lm.last_decode_schedule
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


def test_an_evicted_message_comes_back_with_its_row():
    rng = np.random.default_rng(21)
    ctxs = [rng.integers(0, 511, size=n).tolist() for n in range(25, 33)]
    # the page-exact pool of tests/test_gpu_context_batch.py: 48-byte payloads reach a third page, the pool holds 20
    bits = _bits([48] * 8, seed0=700)
    qs = [QS[i] for i in (0, 3, 0, 3, 0, 3, 0, 3)]  # 300 or 500 candidates: covers of 39 tokens and more
    ref_lm = _provider()
    ref = [ref_lm.encode_batch([b], c, quality=q)[0] for b, c, q in zip(bits, ctxs, qs)]
    assert min(map(len, ref)) >= 39, "covers too short to need a third page: pick longer payloads"
    assert sum(a != b for a, b in zip(ref_lm.encode_batch(bits, contexts=ctxs, quality=qs[0]), ref)) >= 4
    del ref_lm
    lm = _provider()
    lm.lm.kv_segment_pages = 1
    pool = lm.lm.page_pool()
    cap_pages = 20
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got = lm.encode_batch(bits, contexts=ctxs, qualities=qs)
    assert lm.last_schedule["evictions"] > 0, lm.last_schedule
    assert got == ref
    out = lm.decode_batch(got, contexts=ctxs, qualities=qs)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


def test_topk_beyond_the_single_pass_limit_is_grouped_in_the_callers_order(provider_reference):
    lm, context, bits, qs, ref = provider_reference
    wide = {"temp": 1.0, "precision": 16, "topk": 50000}  # the api default
    qs2 = list(qs)
    qs2[2] = wide
    ref2 = list(ref)
    ref2[2] = lm.encode_batch([bits[2]], context, quality=wide)[0]
    lm.drain_states()
    lm._decode_states.clear()
    got, stats = lm.encode_batch(bits, context, qualities=qs2, slots=3, return_stats=True)
    assert got == ref2 and len(stats) == 7 and all(s is not None for s in stats)
    assert lm.last_schedule["quality_groups"] == 2
    want = [len(x).to_bytes(8, "big") for x in bits]
    assert [s["residual_bits"] for s in lm.drain_states()] == want
    assert [s["residual_bits"] for s in lm._decode_states] == want
    lm._decode_states.clear()
    out = lm.decode_batch(got, context, qualities=qs2, slots=3)
    assert lm.last_decode_schedule["quality_groups"] == 2
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


def test_equal_qualities_take_the_one_quality_path(provider_reference):
    lm, context, bits, qs, _ = provider_reference
    ref = lm.encode_batch(bits, context, quality=qs[1])
    before = set(lm._ctx_cache)
    assert lm.encode_batch(bits, context, qualities=[dict(qs[1]) for _ in bits]) == ref
    assert set(lm._ctx_cache) == before  # no "mixed" coder context was made


def test_non_native_lm_steps_the_same_rows_in_lockstep():
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    lm = HipArithmeticLM(_tiny(), None, logits_dtype="f32", compute_dtype=torch.float32)
    assert not lm.lm.native
    a, b = _contexts()[1], _contexts()[3]
    ctxs = [a, b, b, a, b]
    bits = _bits([4, 9, 6, 11, 5])
    qs = [QS[i] for i in (0, 1, 2, 3, 1)]
    ref = [lm.encode_batch([x], c, quality=q)[0] for x, c, q in zip(bits, ctxs, qs)]
    assert lm.encode_batch(bits, contexts=ctxs, qualities=qs) == ref
    same = lm.encode_batch(bits, a, qualities=qs)
    assert same == [lm.encode_batch([x], a, quality=q)[0] for x, q in zip(bits, qs)]
    out = lm.decode_batch(same, a, qualities=qs)
    assert all(o[: len(x)] == x for o, x in zip(out, bits))
    assert any(k[-1] == "mixed" for k in lm._ctx_cache)


def test_qualities_keyword_is_validated(provider_reference):
    lm, context, _, _, _ = provider_reference
    bits = _bits([4, 5])
    q2 = [QS[0], QS[1]]
    bad = (dict(), dict(quality=QS[0], qualities=q2), dict(qualities=q2[:1]), dict(qualities=q2 + q2),
           dict(qualities=[QS[0], dict(QS[1], finish_sent=True)]), dict(qualities=[QS[0], dict(QS[1], temp=0.0)]))
    for kw in bad:
        with pytest.raises(ConfigurationError):
            lm.encode_batch(bits, context, **kw)
        with pytest.raises(ConfigurationError):
            lm.decode_batch([[1, 2], [3]], context, **kw)


def test_stego_batch_round_trips_three_messages_with_three_qualities():
    from neuralsteganography_amd.stego import stego_decode, stego_decode_batch, stego_encode_batch

    lm = _provider()  # ByteTokenizer over the 512-id vocabulary
    qs = [dict(QS[0], finish_sent=False), {"temperature": 0.7, "precision": 16, "top_k": 40, "finish_sent": False},
          dict(QS[3], finish_sent=False)]
    msgs = [b"per-message quality, two packets", bytes(range(40)), b"a third message of two packets"]
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", qualities=qs, seed_text="Dear Alice, ", lm=lm)
    assert [len(r) for r in res] == [2, 2, 2] and lm.last_schedule["quality_groups"] == 1
    assert stego_decode_batch(res, ecc="none", qualities=qs, seed_text="Dear Alice, ", lm=lm) == msgs
    for i in range(3):  # each message alone with its own quality, as the reference's receiver decodes it
        assert stego_decode(res[i], ecc="none", quality=qs[i], seed_text="Dear Alice, ", lm=lm) == msgs[i]
    with pytest.raises(ConfigurationError):
        stego_encode_batch(msgs, ecc="none", quality=qs[0], qualities=qs, lm=lm)
    with pytest.raises(ConfigurationError):
        stego_encode_batch(msgs, ecc="none", qualities=qs[:2], lm=lm)
