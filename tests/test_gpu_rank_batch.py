"""GPU: ``HipRankLM.encode_batch`` / ``decode_batch`` with one context and one quality (temperature and policy) per
message, as ONE slot-scheduled batch on the native step (``RankSlotEncoder`` / ``RankSlotDecoder``,
``ns_rank_*_step_streams``).  The reference of every assertion is each message alone through the unchanged call
``encode_batch_states([bits_i], ctx_i, quality=q_i)`` (lockstep, contiguous cache): tokens, history and residual bits
exact.  Tiny random GPT-2 (2 layers, 2 heads, 128 wide, 512 ids, 256 positions), fp16 compute and logits."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

QUALITIES = [{}, {"top_k": 40}, {"top_p": 0.9, "temp": 0.8}, {"cap_per_token_bits": 3},
             {"prob_temp": 0.7, "top_k": 60}]
N = 9
SIZES = [12, 3, 7, 10, 4, 9, 5, 11, 6]  # payload bytes


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


def _provider(**kw):
    import torch

    from neuralsteganography_amd.lm.rank import HipRankLM

    return HipRankLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(data: bytes):
    return [(b >> k) & 1 for b in data for k in range(8)]


def _messages():
    """9 payloads of 3-12 bytes; 9 contexts of 3-70 tokens -- 2 and 5 are equal, 0 and 7 share a 64-token prefix;
    the 5 qualities in turn."""
    rng = np.random.default_rng(2024)
    payloads = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in SIZES]
    base = rng.integers(0, 511, size=64).tolist()
    ctxs = [base + rng.integers(0, 511, size=3).tolist(),
            rng.integers(0, 511, size=3).tolist(),
            rng.integers(0, 511, size=21).tolist(),
            rng.integers(0, 511, size=40).tolist(),
            rng.integers(0, 511, size=9).tolist(),
            None,
            rng.integers(0, 511, size=33).tolist(),
            base + rng.integers(0, 511, size=6).tolist(),
            rng.integers(0, 511, size=14).tolist()]
    ctxs[5] = list(ctxs[2])
    assert sorted(map(len, ctxs))[0] == 3 and max(map(len, ctxs)) == 70
    quals = [dict(QUALITIES[i % 5]) for i in range(N)]
    return payloads, ctxs, quals


def _alone(lm, bits, ctxs, quals):
    """Every message alone through the unchanged lockstep call."""
    toks, states = [], []
    for b, c, q in zip(bits, ctxs, quals):
        t, s = lm.encode_batch_states([b], c, quality=q)
        toks.append(t[0])
        states.append(s[0])
    return toks, states


@pytest.fixture(scope="module")
def case():
    """The 9 messages and each one alone (computed once, never modified)."""
    lm = _provider()
    payloads, ctxs, quals = _messages()
    bits = [_bits(p) for p in payloads]
    toks, states = _alone(lm, bits, ctxs, quals)
    assert all(len(t) >= 2 for t in toks)
    for s, p in zip(states, payloads):
        assert sum(s["history"]) == 8 * len(p) and int.from_bytes(s["residual_bits"], "big") == 8 * len(p)
    return lm, payloads, bits, ctxs, quals, toks, states


def _set_mode(lm, mode):
    lm.slot_budget_tokens = 8 if mode == "small_budget" else None  # table and history growth, graph re-capture


@pytest.mark.parametrize("mode", ["graphs", "eager", "small_budget"])
def test_every_message_equals_its_own_lone_call(case, mode):
    lm, payloads, bits, ctxs, quals, toks, states = case
    _set_mode(lm, mode)
    try:
        got, st = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals, slots=4, graphs=mode != "eager")
    finally:
        lm.slot_budget_tokens = None
    assert got == toks
    assert [tuple(s["history"]) for s in st] == [tuple(s["history"]) for s in states]
    assert [s["residual_bits"] for s in st] == [s["residual_bits"] for s in states]
    sched = lm.last_schedule
    assert sched["slots"] == 4 and sched["quality_groups"] == 1 and sched["evictions"] == 0
    assert {"slots", "evictions", "compactions", "kv_pages_peak", "prefill_rows", "prefill_groups", "prefill_shared",
            "quality_groups"} <= set(sched)
    assert lm.lm.pool.free_pages == lm.lm.pool.total


@pytest.mark.parametrize("mode", ["graphs", "eager", "small_budget"])
def test_decode_returns_every_messages_bits(case, mode):
    lm, payloads, bits, ctxs, quals, toks, states = case
    _set_mode(lm, mode)
    try:
        out = lm.decode_batch(toks, contexts=ctxs, qualities=quals, states=states, slots=4, graphs=mode != "eager")
    finally:
        lm.slot_budget_tokens = None
    assert out == bits
    sched = lm.last_decode_schedule
    assert sched["slots"] == 4 and sched["quality_groups"] == 1
    assert lm.lm.pool.free_pages == lm.lm.pool.total


def test_queued_states_are_popped_in_message_order(case):
    lm, payloads, bits, ctxs, quals, toks, states = case
    lm.load_states([])
    lm.drain_states()
    got = lm.encode_batch(bits, contexts=ctxs, qualities=quals, slots=4)
    assert got == toks
    assert [tuple(s["history"]) for s in lm.drain_states()] == [tuple(s["history"]) for s in states]
    assert lm.decode_batch(got, contexts=ctxs, qualities=quals, slots=3) == bits


def test_the_parameters_matter(case):
    """With message 0's quality for everyone, or message 0's context for everyone, most other messages give other
    tokens."""
    lm, payloads, bits, ctxs, quals, toks, _ = case
    same_q, _ = lm.encode_batch_states(bits, contexts=ctxs, qualities=[quals[0]] * N, slots=4)
    assert same_q[0] == toks[0]
    assert sum(a != b for a, b in zip(same_q[1:], toks[1:])) >= 5
    same_c, _ = lm.encode_batch_states(bits, contexts=[ctxs[0]] * N, qualities=quals, slots=4)
    assert same_c[0] == toks[0]
    assert sum(a != b for a, b in zip(same_c[1:], toks[1:])) >= 5
    # a shared context= on this path is that context N times
    shared, _ = lm.encode_batch_states(bits, ctxs[0], qualities=quals, slots=4)
    assert shared == same_c


def test_oracle_replay_of_two_messages(case):
    """A lone stream's logits, captured step by step, fed to the oracle with the message's own temp and quality."""
    import torch

    lm, payloads, bits, ctxs, quals, toks, states = case
    for m in (2, 4):  # top_p + temperature, prob_temp + top_k
        assert ("top_p" in quals[m]) or ("prob_temp" in quals[m])
        rows = []
        logits = lm.lm.prefill(ctxs[m], 1, len(toks[m]) + 1)
        for t, tok in enumerate(toks[m]):
            rows.append(logits[0, :512].float().cpu().numpy())
            if t + 1 < len(toks[m]):
                logits = lm.lm.step(torch.tensor([tok], device="cuda", dtype=torch.long))
        q = {k: v for k, v in quals[m].items() if k != "temp"}
        want, cons = oracle.rank_encode_stream(lambda t: rows[t], payloads[m], temp=quals[m].get("temp", 1.0),
                                               quality=q)
        assert want == toks[m], m
        assert cons == list(states[m]["history"]), m


def test_equal_contexts_and_a_common_prefix_share_pages(case):
    _, payloads, bits, ctxs, quals, toks, _ = case
    lm = _provider()
    on, _ = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)
    sched_on = dict(lm.last_schedule)
    lm.share_prefixes = lm.lm.share_prefixes = False
    no_prefix, _ = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)
    rows_no_prefix = lm.last_schedule["prefill_rows"]
    lm.share_contexts = lm.lm.share_contexts = False
    apart, _ = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)
    rows_apart = lm.last_schedule["prefill_rows"]
    assert on == no_prefix == apart == toks
    assert rows_apart == sum(map(len, ctxs))
    assert rows_no_prefix == sum(map(len, ctxs)) - len(ctxs[5])  # an equal context is prefilled once
    assert sched_on["prefill_rows"] < rows_no_prefix            # ... and the common 64-token prefix once
    assert sched_on["prefix_entries"] > 0 and sched_on["prefix_rows_saved"] > 0
    assert "prefix_entries" not in lm.last_schedule
    assert lm.lm.pool.free_pages == lm.lm.pool.total


def test_compaction_keeps_the_tokens(case):
    lm, _, _, ctxs, quals, _, _ = case
    rng = np.random.default_rng(5)
    sizes = [40, 2, 3, 40, 2, 3, 2, 3, 2]  # two long messages among short ones
    bits = [_bits(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()) for n in sizes]
    ref, ref_states = _alone(lm, bits, ctxs, quals)
    got, st = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)  # slots=None: 9 slots, the queue drains at once
    assert lm.last_schedule["compactions"] > 0 and lm.last_schedule["slots"] == 9
    assert got == ref and [s["history"] for s in st] == [s["history"] for s in ref_states]
    out = lm.decode_batch(got, contexts=ctxs, qualities=quals, states=st)
    assert out == bits and lm.last_decode_schedule["compactions"] > 0


def test_eviction_restarts_a_message_with_the_same_tokens():
    rng = np.random.default_rng(51)
    p, q = rng.integers(0, 511, size=40).tolist(), rng.integers(0, 511, size=28).tolist()
    ctxs = [list(c) for c in (p, q, p, q, p, q, p, q)]
    n = len(ctxs)
    # 60 payload bytes at no more than 9 bits per token (512 ids): at least 54 tokens per cover
    bits = [_bits(rng.integers(0, 256, size=60, dtype=np.uint8).tobytes()) for _ in range(n)]
    quals = [{}, {"top_k": 300, "temp": 0.8}] * 4
    ref, ref_states = _alone(_provider(), bits, ctxs, quals)
    assert min(map(len, ref)) >= 54
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    # pages hold 32 positions.  Admission (context + 17 positions: 57 and 45, two pages each): p's shared full page,
    # one own page per p holder and two per q holder = 1 + 4 + 8 = 13 pages, so all eight are admitted; every cover
    # is at least 54 tokens, so every message goes past position 64 and wants a third page: 1 + 8 + 12 = 21 pages
    # at once, which 18 cannot hold
    cap_pages = 18
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got, st = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)
    sched = lm.last_schedule
    assert sched["evictions"] > 0 and sched["kv_pages_peak"] <= cap_pages and pool.total <= cap_pages, sched
    assert got == ref and [s["history"] for s in st] == [s["history"] for s in ref_states]
    assert pool.free_pages == pool.total
    out = lm.decode_batch(got, contexts=ctxs, qualities=quals, states=st)
    assert out == bits and lm.last_decode_schedule["evictions"] > 0
    assert pool.free_pages == pool.total


def test_errors_name_messages(case):
    import torch

    from neuralsteganography_amd.codec.errors import ArithmeticRangeError, DecodeDivergenceError

    lm, payloads, bits, ctxs, quals, toks, states = case
    none = {"top_k": 1}  # one id left: no capacity
    with pytest.raises(ArithmeticRangeError):
        lm.encode_batch_states([bits[6]], ctxs[6], quality=none)
    bad_q = [dict(q) for q in quals]
    bad_q[6] = none
    with pytest.raises(ArithmeticRangeError, match=r"messages \[6\]"):
        lm.encode_batch_states(bits, contexts=ctxs, qualities=bad_q, slots=4)
    # message 1 (top_k 40: 32 ranks selectable of 512 ids): its second token becomes the row's least likely id
    m = 1
    logits = lm.lm.prefill(ctxs[m], 1, 4)
    logits = lm.lm.step(torch.tensor([toks[m][0]], device="cuda", dtype=torch.long))
    alien = int(logits[0, :512].float().argmin())
    assert alien != toks[m][1]
    tampered = [list(t) for t in toks]
    tampered[m][1] = alien
    with pytest.raises(DecodeDivergenceError):
        lm.decode_batch([tampered[m]], ctxs[m], quality=quals[m], states=[states[m]])
    with pytest.raises(DecodeDivergenceError, match=r"messages \[1\]"):
        lm.decode_batch(tampered, contexts=ctxs, qualities=quals, states=states, slots=4)
    # the provider is usable afterwards
    got, _ = lm.encode_batch_states(bits[:3], contexts=ctxs[:3], qualities=quals[:3], slots=2)
    assert got == toks[:3]


def test_front_end_runs_one_batch(case, monkeypatch):
    from neuralsteganography_amd import stego

    lm = case[0]
    monkeypatch.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")
    msgs = [b"rank", b"batch", b"slots!"]
    seeds = ["one seed", "another, longer seed text", "one seed"]
    quals = [{"top_k": 100}, {"top_p": 0.95, "temp": 0.9}, {}]
    kw = dict(ecc="none", chunk_bytes=8)
    lm.load_states([])
    lm.drain_states()
    alone = []
    for m, s, q in zip(msgs, seeds, quals):
        alone.append([list(sp) for sp in stego.stego_encode(m, quality=q, seed_text=s, lm=lm, **kw)])
    lm.load_states([])
    lm.drain_states()
    calls = {"batch": 0, "one": 0}
    enc_batch, enc_one = lm.encode_batch, lm.encode_arithmetic

    @functools.wraps(enc_batch)  # the front end reads the entry's signature for contexts= / qualities=
    def spy_batch(*a, **k):
        calls["batch"] += 1
        return enc_batch(*a, **k)

    @functools.wraps(enc_one)
    def spy_one(*a, **k):
        calls["one"] += 1
        return enc_one(*a, **k)

    monkeypatch.setattr(lm, "encode_batch", spy_batch)
    monkeypatch.setattr(lm, "encode_arithmetic", spy_one)
    res = stego.stego_encode_batch(msgs, seed_texts=seeds, qualities=quals, lm=lm, **kw)
    assert calls == {"batch": 1, "one": 0}
    assert [[list(sp) for sp in r] for r in res] == alone
    lm.load_states(lm.drain_states())
    assert stego.stego_decode_batch([list(r) for r in res], seed_texts=seeds, qualities=quals, lm=lm, ecc="none") == msgs


def test_fallbacks_return_the_lone_results(case):
    from neuralsteganography_amd import synthetic
    from neuralsteganography_amd.lm.rank import HipRankLM

    lm, payloads, bits, ctxs, quals, toks, states = case
    # a max_context window is not batched here: one lockstep call per distinct (context, quality)
    wq = [{"max_context": 8, "top_k": 50}, {}, {"max_context": 8, "top_k": 50}, {"top_k": 40}]
    ref, ref_states = _alone(lm, bits[:4], ctxs[:4], wq)
    got, st = lm.encode_batch_states(bits[:4], contexts=ctxs[:4], qualities=wq)
    assert got == ref and [s["history"] for s in st] == [s["history"] for s in ref_states]
    assert lm.decode_batch(got, contexts=ctxs[:4], qualities=wq, states=st) == bits[:4]
    # a non-native batched LM: the same grouping (distinct contexts: every group is one stream, as a lone call is)
    def syn():
        return HipRankLM(batched_lm=synthetic.SyntheticBatchedLM(3, 512, 3.0, "f32"))

    slm = syn()
    sq = [QUALITIES[0], QUALITIES[1], QUALITIES[4]]  # (top_p 0.9 leaves these synthetic rows no capacity at step 10)
    sref, sstates = _alone(slm, bits[:3], ctxs[:3], sq)
    sgot, sst = slm.encode_batch_states(bits[:3], contexts=ctxs[:3], qualities=sq)
    assert sgot == sref and [s["history"] for s in sst] == [s["history"] for s in sstates]
    assert slm.decode_batch(sgot, contexts=ctxs[:3], qualities=sq, states=sst) == bits[:3]
    assert not hasattr(slm, "last_schedule")
