"""GPU: different contexts of one call share the KV pages of a common prefix.

The prefix is prefilled once, in 64-row blocks, while anything holds it; every context that begins with it is then
prefilled from its first new row on (``ns_seq_attention_ragged_past`` takes the earlier key blocks from the prefix's
pages).  A split at a multiple of 64 changes no bit of the prefill, the other kernels are row-wise and the decode step
reads by address, so every comparison below is bit equality against each message ALONE with its whole context on the
shared-context path.  What the tests guard is the chain bookkeeping: a table row whose chain is in the wrong order,
positions that do not start at ``past``, a prefix returned to the pool while a holder still reads it, a logits row
taken from the wrong sequence.

The tiny model is the one of ``tests/test_gpu_context_batch.py`` (2 layers, 2 heads, n_embd 128, vocab 512,
n_positions 256, fp16 native); the contexts are the A..G set of ``tests/test_prefix_share_host.py``."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import synthetic  # noqa: E402
from neuralsteganography_amd.lm.kvpages import chain_past, plan_prefixes  # noqa: E402

pytestmark = pytest.mark.gpu

NSTEP = 40
NAMES = "ABCDEG"
SLOTS = np.array([3, 0, 5, 1, 4, 2])


def _context_set(seed=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 511, size=130).tolist()
    ctx = {"A": base[:128] + rng.integers(0, 511, size=5).tolist(),
           "B": base[:128] + rng.integers(0, 511, size=40).tolist(),
           "C": base[:64] + rng.integers(0, 511, size=30).tolist(),
           "D": rng.integers(0, 511, size=70).tolist()}
    ctx["E"] = list(ctx["A"])
    ctx["G"] = base[:128]
    return ctx


CTX = _context_set()
LEN = {k: len(c) for k, c in CTX.items()}
assert LEN == {"A": 133, "B": 168, "C": 94, "D": 70, "E": 133, "G": 128}


def _planned_rows(names):
    """Rows a call over ``names`` runs: every run once, every distinct context's rows after its chain once."""
    chains = plan_prefixes([CTX[k] for k in names])
    runs = {c for ch in chains for c in ch}
    rest = {tuple(CTX[k]): LEN[k] - chain_past(ch) for k, ch in zip(names, chains)}
    return sum(b - a for _, a, b in runs) + sum(rest.values())


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


@pytest.fixture(scope="module")
def model_reference():
    """Every context alone on the shared-context path, fed its slot's own tokens: first logits and NSTEP steps."""
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2

    lm = BatchedGPT2(_tiny(), device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    assert lm.native and lm.prefix_sharing
    rng = np.random.default_rng(33)
    ctxs = [list(CTX[k]) for k in NAMES]
    feed = torch.from_numpy(rng.integers(0, 511, size=(len(NAMES), NSTEP))).cuda()  # a different token per slot
    assert all(len(set(feed[:, t].tolist())) > 1 for t in range(NSTEP))
    ref = []
    for m, c in enumerate(ctxs):
        rows = [lm.prefill(c, 1, NSTEP + 1)[0].clone()]
        for t in range(NSTEP):
            rows.append(lm.step(feed[m, t:t + 1])[0].clone())
        ref.append(torch.stack(rows))
    return lm, ctxs, feed, ref


@pytest.mark.parametrize("mode", ["on", "on_budget70", "off"])
def test_prefix_sharing_then_diverging_steps_equal_each_context_alone(model_reference, mode):
    lm, ctxs, feed, ref = model_reference
    n = len(ctxs)
    on = mode.startswith("on")
    saved = lm.prefill_row_budget, lm.share_prefixes
    if mode.endswith("budget70"):
        lm.prefill_row_budget = 70
    lm.share_prefixes = on
    try:
        lm.begin_slots(n, 0, NSTEP + 1)
        first = lm.prefill_contexts(ctxs, SLOTS)
    finally:
        lm.prefill_row_budget, lm.share_prefixes = saved
    kv = lm.kv
    print(mode, lm.last_prefill)
    if on:
        # runs 64 + 64, A's entry 5, B 40, C 30, D 70, G 64
        assert _planned_rows(NAMES) == 64 + 64 + 5 + 40 + 30 + 70 + 64
        assert lm.last_prefill["rows"] == _planned_rows(NAMES)
        assert lm.last_prefill["shared"] == 2  # A and E hold the equal-context entry
        assert lm.last_prefill["prefix_entries"] == 2
        assert lm.last_prefill["prefix_rows_saved"] == 128 + 128 + 64 + 64  # A's entry, B, C, G
        assert sorted((p.past, p.T) for p in kv.prefixes.values()) == [(0, 64), (64, 128)]
        (e,) = kv.entries.values()
        assert (e.past, e.T) == (128, 133) and e.parent.T == 128
        tab = kv.table.cpu().numpy()
        assert (tab == kv.host).all()
        row = dict(zip(NAMES, SLOTS))
        for k in "BEGC":
            shared = {"B": 4, "E": 4, "G": 2, "C": 2}[k]
            assert tab[row[k], :shared].tolist() == tab[row["A"], :shared].tolist(), k
        own = [int(p) for k in NAMES for p in tab[row[k], kv.nshared[row[k]]:] if p]
        held = [int(p) for x in list(kv.prefixes.values()) + [e] for p in x.pages]
        assert len(set(own + held)) == len(own) + len(held) == kv.in_use
    else:
        # 0.30 as it was: A once for A and E (one run of the entry), every other context whole (one run)
        assert lm.last_prefill == {"rows": 133 + 168 + 94 + 70 + 128, "groups": 2, "shared": 2}
        assert not kv.prefixes and all(x.parent is None for x in kv.entries.values())
    want_len = [LEN[k] for k in NAMES]
    assert kv.lens_host[SLOTS].tolist() == want_len
    for m in range(n):
        assert torch.equal(first[m], ref[m][0]), NAMES[m]
    tok = torch.empty(n, dtype=feed.dtype, device="cuda")
    for t in range(NSTEP):  # tails diverge; every slot crosses a page boundary behind its shared columns
        tok[torch.from_numpy(SLOTS).cuda()] = feed[:, t]
        out = lm.step(tok)
        for m in range(n):
            assert torch.equal(out[SLOTS[m]], ref[m][t + 1]), (NAMES[m], t)
    kv.release(np.arange(n))
    assert not kv.entries and not kv.prefixes and kv.in_use == 0 and lm.pool.free_pages == lm.pool.total


# ----------------------------------------------------------------------------------------------------- provider
Q = {"temp": 0.9, "precision": 26, "topk": 300}
PNAMES = ["A", "B", "C", "D", "E", "G", "B", "C", "A", "G", "D", "B"]
PBYTES = [40, 28, 36, 24, 30, 44, 20, 40, 26, 34, 38, 22]  # holders end at different times


def _provider(**kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(n_bytes, seed0=700):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _pool_is_whole(lm):
    pool = lm.lm.pool
    return pool.free_pages == pool.total and not lm.lm.kv.prefixes and not lm.lm.kv.entries


def _alone(lm, bits, ctxs):
    out = []
    for b, c in zip(bits, ctxs):
        out.append(lm.encode_batch([b], c, quality=Q)[0])
    return out


@pytest.fixture(scope="module")
def provider_reference():
    lm = _provider()
    ctxs = [list(CTX[k]) for k in PNAMES]
    bits = _bits(PBYTES)
    return lm, ctxs, bits, _alone(lm, bits, ctxs)


@pytest.mark.parametrize("S", [4, 12])
def test_encode_and_decode_batch_share_prefixes_and_equal_each_message_alone(provider_reference, S):
    lm, ctxs, bits, ref = provider_reference
    runs = {}
    for on in (True, False):
        lm.share_prefixes = on
        try:
            got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=S)
            sched = dict(lm.last_schedule)
            assert _pool_is_whole(lm)
            out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=S)
            dsched = dict(lm.last_decode_schedule)
            assert _pool_is_whole(lm)
        finally:
            lm.share_prefixes = True
        print(S, on, sched, dsched)
        assert got == ref, on  # the tokens of each message alone with its whole context
        assert all(o[: len(b)] == b for o, b in zip(out, bits)), on
        runs[on] = sched, dsched
    (son, don), (soff, doff) = runs[True], runs[False]
    # off: the counters and key sets of 0.30
    assert "prefix_entries" not in soff and "prefix_entries" not in doff and "prefix_rows_saved" not in soff
    assert son["prefix_entries"] >= 2 and don["prefix_entries"] >= 2
    assert son["prefill_rows"] < soff["prefill_rows"] and don["prefill_rows"] < doff["prefill_rows"]
    if S == 12:  # every message live at once: each run once, each distinct context's remaining rows once
        assert son["prefill_rows"] == don["prefill_rows"] == _planned_rows(PNAMES)
        assert soff["prefill_rows"] == sum(LEN[k] for k in "ABCDG")
        assert son["prefix_entries"] == 2 and son["prefix_rows_saved"] == 128 + 128 + 64 + 64
        # the admission maps strictly fewer pages (4 run pages instead of 4 + 4 + 2 + 2 private copies) and every
        # stream grows alike afterwards
        assert son["kv_pages_peak"] < soff["kv_pages_peak"]
    else:  # refills into freed pages; a prefix is prefilled again only after its last holder has left
        assert son["prefill_shared"] >= 2


def test_eviction_of_a_prefix_sharing_message_gives_the_same_tokens():
    names = ["A", "B", "C", "G", "E"]
    ctxs = [list(CTX[k]) for k in names]
    # 48 bytes are about 47 tokens at about 8.2 bits per token; with at least 20 (checked below) every stream outgrows
    # the pages of its admission (T + 17 positions)
    bits = _bits([48] * 5, seed0=750)
    ref_lm = _provider()
    ref = _alone(ref_lm, bits, ctxs)
    assert min(map(len, ref)) >= 20, "covers too short to need another page: pick longer payloads"
    del ref_lm
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    # admission: runs 2 + 2, A's entry 1, own pages A 1, E 1, B 2, C 2, G 3 = 14 (<= cap - 1: all five are admitted);
    # every stream then wants one more page, 19 in all: not all can take it at once
    cap_pages = 16
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q)
    print(lm.last_schedule)
    assert got == ref
    assert lm.last_schedule["evictions"] > 0 and lm.last_schedule["max_live"] == 5, lm.last_schedule
    assert lm.last_schedule["prefix_entries"] >= 2
    assert lm.last_schedule["kv_pages_peak"] <= cap_pages and pool.total <= cap_pages
    assert _pool_is_whole(lm)
    out = lm.decode_batch(got, contexts=ctxs, quality=Q)
    print(lm.last_decode_schedule)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    assert pool.total <= cap_pages and _pool_is_whole(lm)


def test_an_fp8_cache_shares_no_prefix_and_equals_its_own_run_with_the_switch_off():
    lm = _provider(kv_dtype="fp8")
    assert not lm.lm.prefix_sharing
    ctxs = [list(CTX[k]) for k in PNAMES]
    bits = _bits(PBYTES)
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=12)
    sched = dict(lm.last_schedule)
    assert "prefix_entries" not in sched and "prefix_entries" not in lm.lm.last_prefill
    out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=12)
    assert all(o[: len(b)] == b for o, b in zip(out, bits)) and _pool_is_whole(lm)
    lm.share_prefixes = False
    assert lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=12) == got
    assert dict(lm.last_schedule) == sched


def test_stego_batch_shares_the_common_head_of_its_seed_texts():
    from neuralsteganography_amd.stego import stego_decode_batch, stego_encode_batch

    lm = _provider()  # ByteTokenizer over the 512-id vocabulary
    q = dict(Q, finish_sent=False)
    head = "Minutes of the weekly meeting of the board, held in the usual room, as always: "
    assert len(head.encode()) >= 70
    seeds = [head + "Alice spoke first.", head + "Bob was late again, and said so.", head + "nothing happened"]
    toks = [lm.encode_seed(s) for s in seeds]
    assert all(t[:64] == toks[0][:64] for t in toks)
    msgs = [bytes(range(40)), b"five!", bytes(range(100, 130))]  # 2, 1 and 2 packets of 24 bytes
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", quality=q, seed_texts=seeds, lm=lm)
    assert [len(r) for r in res] == [2, 1, 2]
    assert lm.last_schedule["prefix_entries"] == 1 and lm.last_schedule["prefix_rows_saved"] == 3 * 64
    assert lm.last_schedule["prefill_rows"] == 64 + sum(len(t) - 64 for t in toks)
    assert _pool_is_whole(lm)
    assert stego_decode_batch(res, ecc="none", quality=q, seed_texts=seeds, lm=lm) == msgs
    assert lm.last_decode_schedule["prefix_entries"] == 1 and _pool_is_whole(lm)
