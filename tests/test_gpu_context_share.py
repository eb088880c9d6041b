"""GPU: messages of one call that carry the same context share the context's KV pages (library 0.30).

The context is prefilled once while any of them holds it; a holder's page-table row starts with the shared full pages
and continues with its own, the first of which receives the context's last partial page as a copy
(``ns_kv_copy_rows``).  The fused store writes the same bytes whatever table it stores through, the copy moves bytes
and the decode kernel reads by address, so every comparison below is bit equality against each message ALONE with its
context on the shared-context path.  What the tests guard is the bookkeeping (a tail page that stayed shared, a page
returned to the pool while someone still reads it, an entry's logits given to the wrong slot): none of these faults,
they give wrong tokens.

The tiny model is the one of ``tests/test_gpu_context_batch.py``: 2 layers, 2 heads, n_embd 128, vocab 512,
n_positions 256, fp16 native."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402

pytestmark = pytest.mark.gpu

H, D, NL = 2, 64, 2


# ------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_kv_copy_rows_copies_the_head_rows_of_every_layer_and_nothing_else(kv):
    """One segment of 5 pages, layer-major.  Page 0 is the only source, so a source is never a destination; the
    zero-row entry names page 1 as its destination (it writes nothing, so it does not compete with the one-row copy
    into page 1, and a zero-row entry that copied anything would show there)."""
    fmt = _lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16
    esize = 1 if kv == "fp8" else 2
    block = 2 * H * 32 * D
    g = torch.Generator(device="cuda").manual_seed(5)
    raw = torch.randint(0, 256, (NL * 5 * block * esize,), generator=g, device="cuda", dtype=torch.uint8)
    before = raw.cpu().clone()
    base = raw.data_ptr()
    page = [base + p * block * esize for p in range(5)]
    entries = [(page[0], page[1], 1), (page[0], page[2], 17), (page[0], page[3], 31), (page[0], page[1], 0),
               (page[0], page[4], 32), (0, page[2], 5), (page[0], 0, 5), (page[0], page[0], 7), (page[0], page[3], 33),
               (page[0], page[2], -1)]
    src = torch.tensor([e[0] for e in entries], dtype=torch.int64, device="cuda")
    dst = torch.tensor([e[1] for e in entries], dtype=torch.int64, device="cuda")
    rows = torch.tensor([e[2] for e in entries], dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(n=len(entries), d=D, layers=NL, stride=5 * block, f=fmt, heads=H, s=src.data_ptr()):
        return L.ns_kv_copy_rows(s, dst.data_ptr(), rows.data_ptr(), n, layers, stride, heads, d, f, _stream_handle())

    assert call() == 0
    torch.cuda.synchronize()
    got = raw.cpu().view(NL, 5, 2, H, 32, D * esize)
    want = before.clone().view(NL, 5, 2, H, 32, D * esize)
    for p, r in ((1, 1), (2, 17), (3, 31), (4, 32)):
        want[:, p, :, :, :r] = want[:, 0, :, :, :r]  # K and V, both heads, both layers
        assert torch.equal(got[:, p, :, :, :r], before.view(NL, 5, 2, H, 32, D * esize)[:, 0, :, :, :r]), p
    assert torch.equal(got, want)  # every other byte of the segment is what it was
    assert call(n=0) == 0 and call(n=0, s=None) == 0
    assert call(d=32) == _lib.NS_ERR_UNSUPPORTED
    for bad in (dict(n=-1), dict(layers=0), dict(heads=0), dict(f=2), dict(stride=-8), dict(stride=block - 16),
                dict(stride=5 * block + 4), dict(s=None)):
        assert call(**bad) == _lib.NS_ERR_CONFIG, bad
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu().view_as(want), want)


# -------------------------------------------------------------------------------------------------------- model
NSTEP = 40
LEN = {"a": 65, "b": 33, "c": 64, "d": 100, "e": 31}  # c: no tail; d: a singleton; e: no full page
NAMES = ["a", "b", "a", "a", "c", "c", "d", "e", "e"]
SLOTS = np.array([3, 8, 0, 6, 1, 5, 2, 7, 4])


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


@pytest.fixture(scope="module")
def model_reference():
    """Every slot's context alone on the shared-context path, fed that slot's own tokens: first logits and the
    logits of NSTEP steps."""
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2

    lm = BatchedGPT2(_tiny(), device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    assert lm.native
    rng = np.random.default_rng(31)
    ctx = {k: rng.integers(0, 511, size=n).tolist() for k, n in LEN.items()}
    ctxs = [list(ctx[k]) for k in NAMES]
    feed = torch.from_numpy(rng.integers(0, 511, size=(len(NAMES), NSTEP))).cuda()  # a different token per slot
    assert all(len(set(feed[:, t].tolist())) > 1 for t in range(NSTEP))
    ref = []
    for m, c in enumerate(ctxs):
        rows = [lm.prefill(c, 1, NSTEP + 1)[0].clone()]
        for t in range(NSTEP):
            rows.append(lm.step(feed[m, t:t + 1])[0].clone())
        ref.append(torch.stack(rows))
    return lm, ctxs, feed, ref


def _check_tables(kv):
    from neuralsteganography_amd.lm.kvpages import PAGE_ROWS

    tab = kv.table.cpu().numpy()
    assert (tab == kv.host).all()
    full = [LEN[k] // PAGE_ROWS for k in NAMES]
    for i, ki in enumerate(NAMES):
        for j, kj in enumerate(NAMES):
            if i < j and ki == kj and ki != "d":  # holders of one context: the same full pages
                assert tab[SLOTS[i], : full[i]].tolist() == tab[SLOTS[j], : full[j]].tolist(), (i, j)
    later = [int(p) for i in range(len(NAMES)) for p in tab[SLOTS[i], full[i]:] if p]
    assert len(later) == len(set(later))  # every later column is one slot's alone
    shared = {int(p) for e in kv.entries.values() for p in e.pages}
    assert len(shared) == 3 + 2 + 1 and not shared & set(later)
    for i in range(len(NAMES)):
        s = SLOTS[i]
        append = int(tab[s, kv.lens_host[s] // PAGE_ROWS]) if kv.lens_host[s] // PAGE_ROWS < tab.shape[1] else 0
        assert append not in shared, i  # (0: not mapped yet)


@pytest.mark.parametrize("mode", ["share", "share_budget70", "off", "off_budget70"])
def test_shared_contexts_then_diverging_steps_equal_each_context_alone(model_reference, mode):
    lm, ctxs, feed, ref = model_reference
    n = len(ctxs)
    share = mode.startswith("share")
    saved = lm.prefill_row_budget, lm.share_contexts
    if mode.endswith("budget70"):
        lm.prefill_row_budget = 70
    lm.share_contexts = share
    try:
        lm.begin_slots(n, 0, NSTEP + 1)
        first = lm.prefill_contexts(ctxs, SLOTS)
    finally:
        lm.prefill_row_budget, lm.share_contexts = saved
    if share:
        assert lm.last_prefill["rows"] == 65 + 33 + 64 + 100 + 31
        assert lm.last_prefill["shared"] == 7  # the a, c and e holders; b and d are singletons
        assert sorted(e.T for e in lm.kv.entries.values()) == [31, 64, 65]
        assert lm.kv.in_use == (3 + 2 + 1) + (3 * 1 + 2 * 0 + 2 * 1) + 2 + 4  # entries, holders' tails, b, d
        _check_tables(lm.kv)
    else:
        assert lm.last_prefill["rows"] == sum(LEN[k] for k in NAMES) and lm.last_prefill["shared"] == 0
        assert not lm.kv.entries
    want_len = [LEN[k] for k in NAMES]
    assert lm.kv.lens_host[SLOTS].tolist() == want_len
    assert lm.kv.lens[torch.from_numpy(SLOTS).cuda()].tolist() == want_len
    for m in range(n):
        assert torch.equal(first[m], ref[m][0]), m
    tok = torch.empty(n, dtype=feed.dtype, device="cuda")
    for t in range(NSTEP):  # tails diverge; a (65 -> 105), c (64 -> 104) and e (31 -> 71) cross a page boundary
        tok[torch.from_numpy(SLOTS).cuda()] = feed[:, t]
        out = lm.step(tok)
        for m in range(n):
            assert torch.equal(out[SLOTS[m]], ref[m][t + 1]), (m, t)
    if share:
        _check_tables(lm.kv)
        lm.kv.release(np.arange(n))
        assert not lm.kv.entries and lm.kv.in_use == 0 and lm.pool.free_pages == lm.pool.total


def test_direct_prefill_leaves_no_entry_behind_when_pages_run_out_and_keeps_private_pages_private():
    from neuralsteganography_amd.exceptions import KVCapacityError
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2

    lm = BatchedGPT2(_tiny(), device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    a = np.random.default_rng(61).integers(0, 511, size=65).tolist()
    # a twin whose slot already has private pages: both stay singletons, no entry is opened for one holder
    lm.begin_slots(2, 0, 8)
    assert lm.kv.ensure([0], [65]).size == 0
    first = lm.prefill_contexts([a, list(a)], [0, 1])
    assert lm.last_prefill == {"rows": 130, "groups": 1, "shared": 0} and not lm.kv.entries and lm.kv.in_use == 6
    assert torch.equal(first[0], first[1])
    # a page-exact pool of 4: the entry's 3 pages are taken, then only one of the two holders gets its tail page
    lm.release_cache()
    lm.kv_segment_pages = 1
    pool = lm.page_pool()
    pool.budget_bytes = lambda: (4 - pool.total) * pool.page_bytes
    lm.begin_slots(2, 0, 8)
    with pytest.raises(KVCapacityError):
        lm.prefill_contexts([a, list(a)], [0, 1])
    assert not lm.kv.entries and lm.kv.in_use == 0 and not lm.kv.nch.any() and pool.free_pages == pool.total


# ----------------------------------------------------------------------------------------------------- provider
Q = {"temp": 0.9, "precision": 26, "topk": 300}
PLEN = {"x": 33, "y": 65, "z": 100}
PNAMES = ["x", "y", "y", "x", "z", "y", "x", "x", "y", "z"]
PBYTES = [130, 36, 100, 48, 120, 60, 40, 84, 110, 52]  # holders end at very different times


def _provider(**kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(n_bytes, seed0=900):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _pool_is_whole(lm):
    pool = lm.lm.pool
    return pool.free_pages == pool.total


def _alone(lm, bits, ctxs):
    out = []
    for b, c in zip(bits, ctxs):
        out.append(lm.encode_batch([b], c, quality=Q)[0])
        assert _pool_is_whole(lm)
    return out


def _provider_case(lm):
    rng = np.random.default_rng(41)
    ctx = {k: rng.integers(0, 511, size=n).tolist() for k, n in PLEN.items()}
    ctxs = [list(ctx[k]) for k in PNAMES]
    bits = _bits(PBYTES)
    ref = _alone(lm, bits, ctxs)
    # Cover length: every stream maps a page beyond the pages of its admission (T + 17 positions), so every holder
    # grows behind its shared columns; at about 8.2 bits per token 36 bytes are about 35 tokens, and 32 are needed
    for m, (k, r) in enumerate(zip(PNAMES, ref)):
        T = PLEN[k]
        assert T + len(r) > 32 * -(-(T + 17) // 32), f"message {m}: cover too short, pick longer payloads"
    unshared = {}
    lm.share_contexts = False
    try:
        for S in (10, 3):
            assert lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=S) == ref
            unshared[S] = dict(lm.last_schedule)
            assert unshared[S]["prefill_shared"] == 0 and _pool_is_whole(lm)
            out = lm.decode_batch(ref, contexts=ctxs, quality=Q, slots=S)
            assert all(o[: len(b)] == b for o, b in zip(out, bits)) and _pool_is_whole(lm)
    finally:
        lm.share_contexts = True
    assert unshared[10]["prefill_rows"] == sum(PLEN[k] for k in PNAMES)
    return ctxs, bits, ref, unshared


@pytest.fixture(scope="module")
def provider_reference():
    lm = _provider()
    return (lm,) + _provider_case(lm)


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("S", [10, 3])
def test_encode_and_decode_batch_share_equal_contexts_and_equal_each_message_alone(provider_reference, S, graphs):
    lm, ctxs, bits, ref, unshared = provider_reference
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=S, graphs=graphs)
    sched = dict(lm.last_schedule)
    assert _pool_is_whole(lm)
    out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=S, graphs=graphs)
    dsched = dict(lm.last_decode_schedule)
    assert _pool_is_whole(lm)
    assert got == ref
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    print(S, graphs, sched, dsched, unshared[S])
    if S == 10:
        assert sched["prefill_rows"] == dsched["prefill_rows"] == 33 + 65 + 100
        assert sched["prefill_shared"] == dsched["prefill_shared"] == 10
        assert sched["kv_pages_peak"] < unshared[10]["kv_pages_peak"]
    else:  # refills: a context is prefilled again only after its last holder has left
        assert sched["prefill_rows"] <= unshared[3]["prefill_rows"]
        assert dsched["prefill_rows"] <= unshared[3]["prefill_rows"]
        assert sched["prefill_shared"] >= 10 and dsched["prefill_shared"] >= 10


def test_shared_contexts_with_an_fp8_cache_equal_its_own_alone_runs():
    lm = _provider(kv_dtype="fp8")
    ctxs, bits, ref, unshared = _provider_case(lm)
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=10)
    assert got == ref
    assert lm.last_schedule["prefill_rows"] == 33 + 65 + 100 and lm.last_schedule["prefill_shared"] == 10
    assert lm.last_schedule["kv_pages_peak"] < unshared[10]["kv_pages_peak"] and _pool_is_whole(lm)
    out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=10)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    assert lm.last_decode_schedule["prefill_rows"] == 33 + 65 + 100 and _pool_is_whole(lm)


# ----------------------------------------------------------------------------------------------------- eviction
def test_eviction_of_sharing_messages_gives_the_same_tokens_and_a_context_too_large_raises():
    from neuralsteganography_amd.exceptions import KVCapacityError

    rng = np.random.default_rng(51)
    p, q = rng.integers(0, 511, size=40).tolist(), rng.integers(0, 511, size=28).tolist()
    ctxs = [list(c) for c in (p, q, p, q, p, q, p, q)]
    # 48 bytes = 384 bits at about 8.2 bits per token: about 47 tokens.  With at least 39 (checked below) every
    # stream maps a page beyond its admission pages (T + 17 positions: 57 and 45, two table columns; 40 + 39 and
    # 28 + 39 positions need three)
    bits = _bits([48] * 8, seed0=950)
    ref_lm = _provider()
    ref = _alone(ref_lm, bits, ctxs)
    assert min(map(len, ref)) >= 39, "covers too short to need a third page: pick longer payloads"
    del ref_lm
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    # admission: the entries' 2 + 1 pages, one own page per p holder, two per q holder = 15 (<= cap - 1: all eight are
    # admitted); every holder then wants one more page, 23 in all: not all can take it at once
    cap_pages = 18
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q)
    assert got == ref
    assert lm.last_schedule["evictions"] > 0 and lm.last_schedule["max_live"] == 8, lm.last_schedule
    assert lm.last_schedule["kv_pages_peak"] <= cap_pages and pool.total <= cap_pages
    assert pool.free_pages == pool.total
    out = lm.decode_batch(got, contexts=ctxs, quality=Q)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    assert pool.total <= cap_pages and pool.free_pages == pool.total
    # a shared context that cannot fit: 100 tokens are an entry of 4 pages plus one own page per holder; the device
    # holds 4
    cap_pages = 4
    lm.lm.release_cache()
    lm.lm.kv_segment_pages = 1
    pool = lm.lm.page_pool()
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    c = rng.integers(0, 511, size=100).tolist()
    with pytest.raises(KVCapacityError):
        lm.encode_batch(_bits([4, 4, 4]), contexts=[c, list(c), q], quality=Q)
    with pytest.raises(KVCapacityError):
        lm.decode_batch([[1, 2, 3], [4, 5], [6]], contexts=[c, list(c), q], quality=Q)


# ---------------------------------------------------------------------------------------------------- front end
def test_stego_batch_prefills_every_seed_once_for_all_its_packets():
    from neuralsteganography_amd.stego import stego_decode, stego_decode_batch, stego_encode_batch

    lm = _provider()  # ByteTokenizer over the 512-id vocabulary
    q = dict(Q, finish_sent=False)
    msgs = [bytes(range(60)), b"five!", bytes(range(130))]  # 3, 1 and 6 packets of 24 bytes
    seeds = ["Dear Alice, ", "Minutes of the meeting: the board", "x"]
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", quality=q, seed_texts=seeds, lm=lm)
    assert [len(r) for r in res] == [3, 1, 6]
    # every seed's rows once: those with more than one packet through their entry, the one-packet seed alone
    assert lm.last_schedule["prefill_rows"] == sum(len(lm.encode_seed(s)) for s in seeds)
    assert lm.last_schedule["prefill_shared"] == 3 + 6
    assert _pool_is_whole(lm)
    assert stego_decode_batch(res, ecc="none", quality=q, seed_texts=seeds, lm=lm) == msgs
    assert lm.last_decode_schedule["prefill_rows"] == sum(len(lm.encode_seed(s)) for s in seeds)
    assert _pool_is_whole(lm)
    for i in range(3):
        assert stego_decode(res[i], ecc="none", quality=q, seed_text=seeds[i], lm=lm) == msgs[i]
