"""GPU: ``sample_batch`` with one context, length, temperature, top-k and seed per message, as ONE slot-scheduled
batch on the native step (``SlotSampler``, ``ns_sample_step_streams``).  The reference is each message alone through
the lockstep path (``lm.sample_batch(1, length_i, context_i, temperature=, topk=, seed=seeds[i])``): tokens exact,
statistics within rel 2e-5 / abs 2e-6 (the tolerance ``tests/test_gpu_stream_quality.py`` uses for the same
comparison).  Tiny random GPT-2 (2 layers, 2 heads, 128 wide, 512 ids), fp16 logits."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests import sample_stream_cases as sc

pytestmark = pytest.mark.gpu

KEYS = ("avg_NLL", "avg_KL", "avg_Hq")


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


def _provider(**kw):
    import torch

    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _alone(lm, ctxs, lens, temps, topks, seeds, offs=None):
    """Every message alone through the unchanged lockstep path."""
    toks, stats = [], []
    for i in range(len(ctxs)):
        t, s = lm.sample_batch(1, lens[i], ctxs[i], temperature=temps[i], topk=topks[i], seed=seeds[i],
                               stream_offset=offs[i] if offs is not None else 0)
        toks.append(t[0])
        stats.append(s[0])
    return toks, stats


def _close(got, ref):
    for m, (g, r) in enumerate(zip(got, ref)):
        for k in KEYS:
            assert g[k] == pytest.approx(r[k], rel=2e-5, abs=2e-6), (m, k)


@pytest.fixture(scope="module")
def case():
    """The 7 messages and each one alone (computed once, never modified)."""
    lm = _provider()
    ctxs = sc.contexts()
    temps, topks = [p[0] for p in sc.PAIRS], [p[1] for p in sc.PAIRS]
    ref = _alone(lm, ctxs, sc.LENGTHS, temps, topks, sc.SEEDS)
    assert [len(t) for t in ref[0]] == list(sc.LENGTHS)
    kw = dict(contexts=ctxs, lengths=list(sc.LENGTHS), temperatures=temps, topks=topks)
    return lm, ctxs, temps, topks, kw, ref


@pytest.mark.parametrize("mode", ["graphs", "eager", "small_budget"])
def test_every_message_equals_its_own_lone_call(case, mode):
    lm, ctxs, temps, topks, kw, ref = case
    lm.slot_budget_tokens = 8 if mode == "small_budget" else None  # table and history growth, graph re-capture
    try:
        toks, stats = lm.sample_batch(7, 0, seeds=list(sc.SEEDS), slots=3, graphs=mode != "eager", **kw)
    finally:
        lm.slot_budget_tokens = None
    assert toks == ref[0]
    _close(stats, ref[1])
    sched = lm.last_sample_schedule
    assert sched["slots"] == 3 and sched["quality_groups"] == 1
    assert set(sched) == {"slots", "quality_groups", "prefill_rows", "compactions", "evictions", "kv_pages_peak"}
    assert sched["prefill_rows"] == sum(sc.CONTEXT_LENGTHS) and sched["evictions"] == 0
    assert lm.lm.pool.free_pages == lm.lm.pool.total


def test_the_first_messages_parameters_give_other_tokens(case):
    """The rows matter: with message 0's temperature, top-k and seed for everyone the other messages differ."""
    lm, ctxs, temps, topks, kw, ref = case
    toks, _ = lm.sample_batch(7, 0, contexts=ctxs, lengths=list(sc.LENGTHS), temperatures=[temps[0]] * 7,
                              topks=[topks[0]] * 7, seeds=[sc.SEEDS[0]] * 7, slots=3)
    assert toks[0] == ref[0][0]
    assert sum(a != b for a, b in zip(toks[1:], ref[0][1:])) >= 5


def test_one_shared_seed_draws_as_stream_offset_plus_message(case):
    lm, ctxs, temps, topks, kw, _ = case
    seed, off = 99, 4
    ref = _alone(lm, ctxs, sc.LENGTHS, temps, topks, [seed] * 7, offs=[off + i for i in range(7)])
    toks, stats = lm.sample_batch(7, 0, seed=seed, stream_offset=off, slots=4, **kw)
    assert toks == ref[0]
    _close(stats, ref[1])
    # the all-scalar slot call is a special case of the same rule, and equals the lockstep call
    lock = lm.sample_batch(5, 9, ctxs[4], temperature=0.9, topk=40, seed=7, stream_offset=2)
    slot = lm.sample_batch(5, 9, ctxs[4], temperature=0.9, topk=40, seed=7, stream_offset=2, slots=2)
    assert slot[0] == lock[0]
    _close(slot[1], lock[1])


def test_oracle_replay_of_two_messages(case):
    """A lone stream's logits, captured step by step and fed to the oracle with the message's own parameters."""
    import torch

    lm, ctxs, temps, topks, kw, ref = case
    for m in (1, 4):
        st = oracle.new_state(1)
        logits = lm.lm.prefill(ctxs[m], 1, sc.LENGTHS[m] + 1)
        toks = []
        for t in range(sc.LENGTHS[m]):
            row = logits[0, :512].float().cpu().numpy()
            tok, _ = oracle.sample_step(row, st, banned=[511], temp=temps[m], topk=topks[m], seed=sc.SEEDS[m], gid=0)
            toks.append(tok)
            if t + 1 < sc.LENGTHS[m]:
                logits = lm.lm.step(torch.tensor([tok], device="cuda", dtype=torch.long))
        assert toks == ref[0][m], m


def test_equal_contexts_and_a_common_prefix_share_pages():
    lm = _provider()
    rng = np.random.default_rng(77)
    base = rng.integers(0, 511, size=64).tolist()
    a, b = base + rng.integers(0, 511, size=10).tolist(), base + rng.integers(0, 511, size=20).tolist()
    ctxs = [a, b, list(a), rng.integers(0, 511, size=33).tolist(), list(b)]
    kw = dict(contexts=ctxs, lengths=[20, 6, 9, 4, 18], temperatures=[1.0, 0.8, 1.2, 1.0, 0.9],
              topks=[40, 300, 2, 40, 100], seeds=[1, 2, 3, 4, 5])
    on = lm.sample_batch(5, 0, **kw)
    rows_on = lm.last_sample_schedule["prefill_rows"]
    lm.share_prefixes = False
    no_prefix = lm.sample_batch(5, 0, **kw)
    rows_no_prefix = lm.last_sample_schedule["prefill_rows"]
    lm.share_contexts = False
    apart = lm.sample_batch(5, 0, **kw)
    rows_apart = lm.last_sample_schedule["prefill_rows"]
    assert on[0] == no_prefix[0] == apart[0]
    _close(on[1], apart[1])
    assert rows_apart == sum(map(len, ctxs))
    assert rows_no_prefix == len(a) + len(b) + 33  # an equal context is prefilled once
    assert rows_on < rows_no_prefix  # ... and the common 64-token prefix once
    assert lm.lm.pool.free_pages == lm.lm.pool.total


def test_compaction_keeps_the_tokens():
    lm = _provider()
    ctxs = sc.contexts()
    lens = [60, 3, 4, 60, 2, 5, 3]  # two long messages among short ones
    temps, topks = [p[0] for p in sc.PAIRS], [p[1] for p in sc.PAIRS]
    ref = _alone(lm, ctxs, lens, temps, topks, sc.SEEDS)
    toks, stats = lm.sample_batch(7, 0, contexts=ctxs, lengths=lens, temperatures=temps, topks=topks,
                                  seeds=list(sc.SEEDS))  # slots=None: 7 slots, the queue is drained at once
    assert lm.last_sample_schedule["compactions"] > 0 and lm.last_sample_schedule["slots"] == 7
    assert toks == ref[0]
    _close(stats, ref[1])


def test_eviction_restarts_a_message_with_the_same_tokens():
    rng = np.random.default_rng(51)
    p, q = rng.integers(0, 511, size=40).tolist(), rng.integers(0, 511, size=28).tolist()
    ctxs = [list(c) for c in (p, q, p, q, p, q, p, q)]
    n = len(ctxs)
    lens, temps, topks, seeds = [50] * n, [1.0, 0.8] * 4, [40, 300] * 4, list(range(21, 21 + n))
    ref = _alone(_provider(), ctxs, lens, temps, topks, seeds)
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    # admission (context + 17 positions: 57 and 45, two pages each): p's shared full page, one own page per p holder
    # and two per q holder = 13 pages; every message then draws past position 64 and wants a third page, 21 in all
    cap_pages = 18
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    toks, stats = lm.sample_batch(n, 0, contexts=ctxs, lengths=lens, temperatures=temps, topks=topks, seeds=seeds)
    sched = lm.last_sample_schedule
    assert sched["evictions"] > 0 and sched["kv_pages_peak"] <= cap_pages and pool.total <= cap_pages, sched
    assert toks == ref[0]
    _close(stats, ref[1])
    assert pool.free_pages == pool.total


def test_fp8_cache_equals_its_own_lone_calls():
    lm = _provider(kv_dtype="fp8")
    ctxs = sc.contexts()[2:6]
    lens, temps, topks, seeds = [12, 3, 20, 7], [1.0, 0.7, 1.3, 0.9], [40, 2, 300, 100], [8, 9, 10, 11]
    ref = _alone(lm, ctxs, lens, temps, topks, seeds)
    toks, stats = lm.sample_batch(4, 0, contexts=ctxs, lengths=lens, temperatures=temps, topks=topks, seeds=seeds,
                                  slots=2)
    assert toks == ref[0]
    _close(stats, ref[1])


def test_code_base_sample_batch(case):
    from neuralsteganography_amd import code_base

    lm, ctxs, temps, topks, kw, ref = case
    got = code_base.sample_batch(lm, None, 0, None, 7, seeds=list(sc.SEEDS), **kw)
    for m, g in enumerate(got):
        one = code_base.sample(lm, None, sc.LENGTHS[m], ctxs[m], temperature=temps[m], topk=topks[m], seed=sc.SEEDS[m])
        assert g[0] == one[0] == ref[0][m]
        assert g[1:] == pytest.approx(one[1:], rel=2e-5, abs=2e-6)
    # none of the new keywords: the lockstep path, exactly
    plain = code_base.sample_batch(lm, None, 6, ctxs[5], 3, temperature=0.9, topk=40, seed=9)
    t, s = lm.sample_batch(3, 6, ctxs[5][-1022:], temperature=0.9, topk=40, seed=9)
    assert plain == [(t[i], s[i]["avg_NLL"], s[i]["avg_KL"], s[i]["avg_Hq"]) for i in range(3)]
    assert len(plain) == 3 and all(len(x[0]) == 6 for x in plain)


def test_topk_beyond_the_limit_runs_as_a_second_group(case):
    lm, ctxs, temps, _, _, _ = case
    topks = [40, -1, 40, -1, 300, -1, 2]
    ref = _alone(lm, ctxs, sc.LENGTHS, temps, topks, sc.SEEDS)
    toks, stats = lm.sample_batch(7, 0, contexts=ctxs, lengths=list(sc.LENGTHS), temperatures=temps, topks=topks,
                                  seeds=list(sc.SEEDS), slots=3)
    assert lm.last_sample_schedule["quality_groups"] == 2
    assert toks == ref[0]
    _close(stats, ref[1])
