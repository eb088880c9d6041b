"""GPU: one context per message in one batch (``encode_batch(contexts=...)``, ``stego_encode_batch(seed_texts=...)``;
the reference's unit of work is one message with its own ``seed_text``, ``src/neuralstego/api.py:707-747``).

The contract: a message's tokens do not depend on how its context reached the cache -- prefilled ragged into the
stream's own KV pages (``ns_seq_attention_ragged``, ``BatchedGPT2.prefill_contexts``) or kept once as the shared
prefix of a one-message call -- because the receiver decodes alone with ``decode_arithmetic(tokens, context)``.
Every comparison below is bit equality (``torch.equal`` / equal token lists) against the existing shared-context path
or the existing ``ns_seq_attention``; the one tolerance (2e-3 absolute against an fp32 softmax) is the bound
``tests/test_gpu_lm_kernels.py::test_seq_attention_matches_fp32_reference`` uses for this arithmetic.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import ragged_blocks  # noqa: E402

pytestmark = pytest.mark.gpu

H, D = 2, 64
C = H * D
LENS = [1, 15, 16, 17, 63, 64, 65, 130]
ORDER = [5, 0, 7, 2, 4, 1, 6, 3]  # the packing order of LENS (shuffled)


def _q8(t):
    out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    assert _lib.lib().ns_quantize_fp8(t.contiguous().data_ptr(), out.data_ptr(), t.numel(), _stream_handle()) == 0
    return out


def _ragged(qkv, lens, table=None, seq_slot=None, layer_off=0, fmt=0):
    seq_start, blocks = ragged_blocks(lens)
    R = int(seq_start[-1])
    out = torch.full((R, C), 7.0, device="cuda", dtype=torch.float16)
    ds, db = torch.from_numpy(seq_start).cuda(), torch.from_numpy(blocks).cuda()
    rc = _lib.lib().ns_seq_attention_ragged(
        qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), ds.data_ptr(), len(lens), R, db.data_ptr(),
        blocks.shape[0], H, D, D ** -0.5, table.data_ptr() if table is not None else None,
        table.stride(0) if table is not None else 0, table.shape[1] if table is not None else 0,
        seq_slot.data_ptr() if seq_slot is not None else None, table.shape[0] if table is not None else 0, layer_off,
        fmt, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out, seq_start


def _seq_attn(qkv, T):
    o = torch.empty((T, C), device="cuda", dtype=torch.float16)
    rc = _lib.lib().ns_seq_attention(qkv.data_ptr(), qkv.stride(0), o.data_ptr(), o.stride(0), 1, T, H, D, D ** -0.5,
                                     _stream_handle())
    assert rc == 0
    return o


@pytest.fixture(scope="module")
def packed():
    lens = [LENS[i] for i in ORDER]
    g = torch.Generator(device="cuda").manual_seed(77)
    qkv = torch.randn((sum(lens), 3 * C), generator=g, device="cuda").half()
    out, seq_start = _ragged(qkv, lens)
    return lens, qkv, out, seq_start


def test_ragged_rows_equal_the_sequence_alone_and_ignore_the_other_sequences(packed):
    lens, qkv, out, seq_start = packed
    assert sorted(lens) == LENS
    for s, T in enumerate(lens):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        alone = _seq_attn(qkv[a:b].contiguous(), T)
        assert torch.equal(out[a:b], alone), (s, T)
        # every OTHER sequence's rows NaN: a cross-sequence read would reach this sequence's rows as NaN (a masked
        # key contributes 0 x NaN = NaN to the PV product)
        poisoned = torch.full_like(qkv, float("nan"))
        poisoned[a:b] = qkv[a:b]
        got, _ = _ragged(poisoned, lens)
        assert torch.equal(got[a:b], alone), (s, T)


def test_ragged_matches_fp32_reference(packed):
    lens, qkv, out, seq_start = packed
    for s, T in enumerate(lens):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        x = qkv[a:b].float().view(T, 3, H, D)
        q, k, v = (x[:, i].transpose(0, 1) for i in range(3))
        sc = (q @ k.transpose(-1, -2)) * D ** -0.5
        sc = sc.masked_fill(torch.triu(torch.ones(T, T, device="cuda", dtype=torch.bool), 1), float("-inf"))
        ref = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(T, C)
        err = (out[a:b].float() - ref).abs().max().item()
        print(f"T={T}: max abs error {err:.3e}")
        assert err < 2e-3, (T, err)


def test_ragged_entry_point_refuses_bad_arguments(packed):
    lens, qkv, _, _ = packed
    seq_start, blocks = ragged_blocks(lens)
    ds, db = torch.from_numpy(seq_start).cuda(), torch.from_numpy(blocks).cuda()
    out = torch.empty((qkv.shape[0], C), device="cuda", dtype=torch.float16)
    tab = torch.zeros((8, 5), dtype=torch.int64, device="cuda")
    slot = torch.arange(8, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(qkv=qkv.data_ptr(), ldq=qkv.stride(0), out=out.data_ptr(), ldo=C, ds=ds.data_ptr(), n=len(lens),
                 R=qkv.shape[0], db=db.data_ptr(), nblk=blocks.shape[0], H=H, D=D, tab=tab.data_ptr(), ts=5, mc=5,
                 slot=slot.data_ptr(), ns=8, lo=0, fmt=0)
        a.update(kw)
        return _lib.lib().ns_seq_attention_ragged(a["qkv"], a["ldq"], a["out"], a["ldo"], a["ds"], a["n"], a["R"],
                                                  a["db"], a["nblk"], a["H"], a["D"], D ** -0.5, a["tab"], a["ts"],
                                                  a["mc"], a["slot"], a["ns"], a["lo"], a["fmt"], _stream_handle())

    assert call() == 0  # (an all-zero table: nothing stored)
    assert call(D=32) == _lib.NS_ERR_UNSUPPORTED
    for bad in (dict(qkv=None), dict(ds=None), dict(db=None), dict(n=0), dict(nblk=0), dict(ldq=3 * C - 8),
                dict(ldo=C - 4), dict(nblk=10 ** 6), dict(slot=None), dict(mc=0), dict(ts=4), dict(fmt=2), dict(lo=-8),
                dict(lo=4), dict(ns=0), dict(R=3)):
        assert call(**bad) == _lib.NS_ERR_CONFIG, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_ragged_stores_every_row_once_into_the_streams_pages_and_nothing_else(packed, kv):
    lens, qkv, attn, seq_start = packed
    n_layer, layer = 2, 1
    rng = np.random.default_rng(5)
    dt = torch.uint8 if kv == "fp8" else torch.float16
    fmt = _lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16
    need = [-(-T // 32) for T in lens]
    npages = 2 * (sum(need) + 1) + 1  # odd pages are used (permuted), even ones are guards; one spare used page
    pool = torch.empty((npages, n_layer, 2, H, 32, D), dtype=dt, device="cuda")
    pool.view(torch.uint8).fill_(0xA5)
    sentinel = pool.clone()
    page_bytes = pool[0].numel() * pool.element_size()
    used = rng.permutation(np.arange(1, npages, 2))
    n_slots = len(lens) + 3
    slots = rng.permutation(n_slots)[: len(lens)]
    table = np.zeros((n_slots, max(need) + 1), dtype=np.int64)  # the entry after a stream's last page stays 0
    page_of = {}
    k = 0
    for s, nch in enumerate(need):
        for c in range(nch):
            page_of[(s, c)] = int(used[k])
            table[slots[s], c] = pool.data_ptr() + int(used[k]) * page_bytes
            k += 1
    kcol = qkv[:, C:2 * C].contiguous().view(-1, H, D)
    vcol = qkv[:, 2 * C:].contiguous().view(-1, H, D)
    if kv == "fp8":
        kcol, vcol = _q8(kcol), _q8(vcol)

    def expected(skip=()):
        want = sentinel.clone()
        for s, T in enumerate(lens):
            a = int(seq_start[s])
            for c in range(need[s]):
                if (s, c) in skip:
                    continue
                r0, r1 = 32 * c, min(32 * c + 32, T)
                want[page_of[(s, c)], layer, 0, :, : r1 - r0] = kcol[a + r0:a + r1].transpose(0, 1)
                want[page_of[(s, c)], layer, 1, :, : r1 - r0] = vcol[a + r0:a + r1].transpose(0, 1)
        return want

    d_slot = torch.from_numpy(slots.astype(np.int32)).cuda()
    layer_off = layer * 2 * H * 32 * D
    out, _ = _ragged(qkv, lens, torch.from_numpy(table).cuda(), d_slot, layer_off, fmt)
    assert torch.equal(out, attn)  # the store does not touch the attention
    # stored rows = the K / V columns (fp8: ns_quantize_fp8 of them); every other byte still the sentinel: rows past
    # a sequence's end in its last page, layer 0's blocks, guard pages, the spare page
    assert torch.equal(pool.view(torch.uint8), expected().view(torch.uint8))
    # one table entry zeroed: those rows are absent, everything else as before
    big = lens.index(130)
    table2 = table.copy()
    table2[slots[big], 1] = 0
    pool.copy_(sentinel)
    out, _ = _ragged(qkv, lens, torch.from_numpy(table2).cuda(), d_slot, layer_off, fmt)
    assert torch.equal(out, attn)
    assert torch.equal(pool.view(torch.uint8), expected(skip={(big, 1)}).view(torch.uint8))


# --------------------------------------------------------------------- decode attention: prefix rows vs own pages
@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("B,T", [(600, 32), (600, 33), (600, 100), (5, 65)])
def test_decode_attention_bits_do_not_depend_on_where_the_context_rows_live(kv, B, T):
    """``ns_decode_attention_paged`` with the context's T rows as the shared prefix (T0 = T) against the same rows at
    the head of every stream's own pages (T0 = 0): the same bits.  B = 600 x 2 heads is the 8-pair workgroup form
    (its short-key path takes the context's first chunk from the prefix when T0 >= 32), B = 5 the one-pair form; own
    lengths 0..220 cross the one-wave / two-wave split at 256 keys."""
    g = torch.Generator(device="cuda").manual_seed(B + T)
    rng = np.random.default_rng(B + T)
    own = rng.integers(0, 221, size=B)
    own[0], own[1] = 0, 220
    fmt = _lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16
    qkv = torch.randn((B, 3 * C), generator=g, device="cuda").half()
    ck = torch.randn((H, T, D), generator=g, device="cuda").half()
    cv = torch.randn((H, T, D), generator=g, device="cuda").half()
    rows = int(own.max()) + 1
    ok = torch.randn((B, H, rows, D), generator=g, device="cuda").half()
    ov = torch.randn((B, H, rows, D), generator=g, device="cuda").half()
    if kv == "fp8":
        ck, cv, ok, ov = _q8(ck), _q8(cv), _q8(ok), _q8(ov)
    lens = torch.from_numpy((T + own).astype(np.int32)).cuda()

    def run(T0):
        # stream rows: the own rows, preceded by the context when it is not the prefix
        sk = ok if T0 else torch.cat([ck[None].expand(B, -1, -1, -1), ok], dim=2)
        sv = ov if T0 else torch.cat([cv[None].expand(B, -1, -1, -1), ov], dim=2)
        nch = -(-(sk.shape[2] + 1) // 32)
        pad = torch.zeros((B, H, nch * 32 - sk.shape[2], D), dtype=sk.dtype, device="cuda")
        sk, sv = torch.cat([sk, pad], dim=2), torch.cat([sv, pad], dim=2)
        # pages [B * nch][K|V][H][32][D], stream b's chunk c at page perm[b * nch + c]
        perm = torch.from_numpy(rng.permutation(B * nch)).cuda()
        pool = torch.empty((B * nch, 2, H, 32, D), dtype=sk.dtype, device="cuda")
        pool[perm, 0] = sk.view(B, H, nch, 32, D).permute(0, 2, 1, 3, 4).reshape(B * nch, H, 32, D)
        pool[perm, 1] = sv.view(B, H, nch, 32, D).permute(0, 2, 1, 3, 4).reshape(B * nch, H, 32, D)
        page_bytes = pool[0].numel() * pool.element_size()
        table = (pool.data_ptr() + perm.view(B, nch) * page_bytes).contiguous()
        out = torch.full((B, C), 7.0, device="cuda", dtype=torch.float16)
        rc = _lib.lib().ns_decode_attention_paged(
            qkv.data_ptr(), qkv.stride(0), table.data_ptr(), table.stride(0), nch, 0,
            ck.data_ptr() if T0 else None, cv.data_ptr() if T0 else None, ck.stride(0) if T0 else 0, T0, B, H, D,
            lens.data_ptr(), 0, fmt, None, 0, None, out.data_ptr(), out.stride(0), D ** -0.5, _stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        return out

    shared, paged = run(T), run(0)
    assert torch.isfinite(shared.float()).all()
    assert torch.equal(shared, paged)


# ------------------------------------------------------------------------------------------------------- model
CTX_LENS = [1, 31, 32, 33, 64, 65, 100]
NSTEP = 40


def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


def _contexts(seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 511, size=n).tolist() for n in CTX_LENS]


@pytest.fixture(scope="module")
def model_reference():
    """Every context alone on the shared-context path: first logits and the logits of NSTEP fed tokens."""
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2

    lm = BatchedGPT2(_tiny(), device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    assert lm.native
    ctxs = _contexts()
    feed = torch.from_numpy(np.random.default_rng(12).integers(0, 511, size=NSTEP)).cuda()
    ref = []
    for c in ctxs:
        rows = [lm.prefill(c, 1, NSTEP + 1)[0].clone()]
        for t in range(NSTEP):
            rows.append(lm.step(feed[t:t + 1])[0].clone())
        ref.append(torch.stack(rows))
    return lm, ctxs, feed, ref


@pytest.mark.parametrize("row_budget", [None, 70])
def test_prefill_contexts_then_steps_equal_each_context_alone(model_reference, row_budget):
    lm, ctxs, feed, ref = model_reference
    n = len(ctxs)
    slots = np.array([3, 0, 6, 1, 5, 2, 4])
    saved = lm.prefill_row_budget
    if row_budget is not None:
        lm.prefill_row_budget = row_budget
    try:
        lm.begin_slots(n, 0, NSTEP + 1)
        first = lm.prefill_contexts(ctxs, slots)
    finally:
        lm.prefill_row_budget = saved
    assert lm.last_prefill["rows"] == sum(CTX_LENS)
    assert lm.last_prefill["groups"] == (1 if row_budget is None else 5)  # [1, 31, 32] [33] [64] [65] [100] at 70 rows
    assert lm.kv.lens_host[slots].tolist() == CTX_LENS and lm.kv.lens[torch.from_numpy(slots).cuda()].tolist() == CTX_LENS
    for m in range(n):
        assert torch.equal(first[m], ref[m][0]), m
    for t in range(NSTEP):  # crosses a page boundary and the 64-key boundary for some streams
        out = lm.step(feed[t].expand(n).contiguous())
        for m in range(n):
            assert torch.equal(out[slots[m]], ref[m][t + 1]), (m, t)


# ---------------------------------------------------------------------------------------------------- provider
Q = {"temp": 0.9, "precision": 26, "topk": 300}


def _provider(**kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(n_bytes, seed0=500):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _alone(lm, bits, ctxs):
    return [lm.encode_batch([b], c, quality=Q)[0] for b, c in zip(bits, ctxs)]


@pytest.fixture(scope="module")
def provider_reference():
    lm = _provider()
    ctxs = _contexts()
    bits = _bits([4, 12, 7, 9, 5, 11, 8])
    return lm, ctxs, bits, _alone(lm, bits, ctxs)


@pytest.mark.parametrize("mode", ["graphs", "eager", "small_budget"])
def test_encode_and_decode_batch_with_contexts_equal_each_message_alone(provider_reference, mode):
    lm, ctxs, bits, ref = provider_reference
    kw = dict(graphs=mode != "eager")
    lm.slot_budget_tokens = 8 if mode == "small_budget" else None  # table growth and graph re-capture
    try:
        got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=3, **kw)  # 7 messages, 3 slots: refills
        sched = dict(lm.last_schedule)
        out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=3, **kw)
        dsched = dict(lm.last_decode_schedule)
    finally:
        lm.slot_budget_tokens = None
    assert got == ref
    assert sched["prefill_rows"] == sum(CTX_LENS) and sched["prefill_groups"] >= 3, sched
    assert dsched["prefill_rows"] == sum(CTX_LENS) and dsched["prefill_groups"] >= 3, dsched
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    if mode == "graphs":  # the receiver's side: each message alone with its own context
        for m in range(len(bits)):
            alone = lm.decode_batch([got[m]], ctxs[m], quality=Q)[0]
            assert alone[: len(bits[m])] == bits[m], m


def test_contexts_with_an_fp8_cache_equal_its_own_shared_path():
    lm = _provider(kv_dtype="fp8")
    ctxs = _contexts()
    bits = _bits([4, 12, 7, 9, 5, 11, 8])
    ref = _alone(lm, bits, ctxs)
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q, slots=3)
    assert got == ref
    out = lm.decode_batch(got, contexts=ctxs, quality=Q, slots=3)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


def test_non_native_lm_runs_once_per_distinct_context_in_the_callers_order():
    """The PyTorch fp32 forward has no pages: messages are grouped by distinct context, each group runs the lockstep
    loop, results (tokens, statistics, the bit-count states) come back in the caller's order."""
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    lm = HipArithmeticLM(_tiny(), None, logits_dtype="f32", compute_dtype=torch.float32)
    assert not lm.lm.native
    a, b = _contexts()[1], _contexts()[3]
    ctxs = [a, b, b, a, b]
    bits = _bits([4, 9, 6, 11, 5])
    ref = [lm.encode_batch([x], c, quality=Q)[0] for x, c in zip(bits, ctxs)]
    lm.drain_states()
    lm._decode_states.clear()
    calls = []
    orig = lm.lm.prefill
    lm.lm.prefill = lambda c, B, n: (calls.append((list(c), B)), orig(c, B, n))[1]
    try:
        got, stats = lm.encode_batch(bits, contexts=ctxs, quality=Q, return_stats=True)
        assert calls == [(a, 2), (b, 3)]
        assert got == ref and len(stats) == 5 and all(s is not None for s in stats)
        want = [len(x).to_bytes(8, "big") for x in bits]
        assert [s["residual_bits"] for s in lm.drain_states()] == want
        assert [s["residual_bits"] for s in lm._decode_states] == want
        out = lm.decode_batch(got, contexts=ctxs, quality=Q)
    finally:
        lm.lm.prefill = orig
    assert all(o[: len(x)] == x for o, x in zip(out, bits))


def test_contexts_keyword_is_validated():
    from neuralsteganography_amd.exceptions import ConfigurationError

    lm = _provider()
    bits = _bits([4, 5])
    c = _contexts()[:2]
    for kw in (dict(), dict(context=c[0], contexts=c), dict(contexts=c[:1]), dict(contexts=c + c)):
        with pytest.raises(ConfigurationError):
            lm.encode_batch(bits, quality=Q, **kw)
        with pytest.raises(ConfigurationError):
            lm.decode_batch([[1, 2], [3]], quality=Q, **kw)


def test_equal_contexts_take_the_shared_path():
    lm = _provider()
    c = _contexts()[6]
    bits = _bits([6, 10, 4, 9])
    ref = lm.encode_batch(bits, c, quality=Q)
    shared = dict(lm.last_schedule)
    got = lm.encode_batch(bits, contexts=[list(c) for _ in bits], quality=Q)
    assert got == ref
    assert lm.last_schedule["prefill_rows"] == 0  # no context rows in the pages
    assert lm.last_schedule["kv_pages_peak"] == shared["kv_pages_peak"]
    out = lm.decode_batch(got, contexts=[list(c) for _ in bits], quality=Q)
    assert all(o[: len(b)] == b for o, b in zip(out, bits)) and lm.last_decode_schedule["prefill_rows"] == 0


def test_eviction_with_contexts_gives_the_same_tokens_and_a_context_too_large_raises():
    from neuralsteganography_amd.exceptions import KVCapacityError

    rng = np.random.default_rng(21)
    ctxs = [rng.integers(0, 511, size=n).tolist() for n in range(25, 33)]  # 25..32 tokens
    # 48 bytes = 384 bits at about log2(300) = 8.2 bits per token of the near-uniform random model: about 47 tokens.
    # With at least 39 (checked below) every stream reaches position 64, its third page; admission maps two
    # (T + 17 <= 49 positions)
    bits = _bits([48] * 8, seed0=700)
    ref_lm = _provider()
    ref = _alone(ref_lm, bits, ctxs)
    assert min(map(len, ref)) >= 39, "covers too short to need a third page: pick longer payloads"
    del ref_lm
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    cap_pages = 20  # all 8 are admitted (16 pages), not all can take a third page at once
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got = lm.encode_batch(bits, contexts=ctxs, quality=Q)
    assert got == ref
    assert lm.last_schedule["evictions"] > 0, lm.last_schedule
    assert lm.last_schedule["prefill_rows"] > sum(map(len, ctxs))  # an evicted message is prefilled again
    assert pool.total <= cap_pages
    out = lm.decode_batch(got, contexts=ctxs, quality=Q)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    # a context that cannot fit alone: 100 tokens need 4 pages, the device holds 2
    cap_pages = 2
    lm.lm.release_cache()
    lm.lm.kv_segment_pages = 1
    pool = lm.lm.page_pool()
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    big = [rng.integers(0, 511, size=100).tolist(), ctxs[0]]
    with pytest.raises(KVCapacityError):
        lm.encode_batch(_bits([4, 4]), contexts=big, quality=Q)
    with pytest.raises(KVCapacityError):
        lm.decode_batch([[1, 2, 3], [4, 5]], contexts=big, quality=Q)


def test_stego_batch_round_trips_three_messages_with_three_seeds():
    from neuralsteganography_amd.stego import stego_decode, stego_decode_batch, stego_encode_batch

    lm = _provider()  # ByteTokenizer over the 512-id vocabulary
    q = dict(Q, finish_sent=False)
    msgs = [b"per-message seeds", bytes(range(40)), b"z"]
    seeds = ["Dear Alice, ", "Minutes of the meeting: the board", "x"]
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", quality=q, seed_texts=seeds, lm=lm)
    assert lm.last_schedule["prefill_rows"] > 0
    assert stego_decode_batch(res, ecc="none", quality=q, seed_texts=seeds, lm=lm) == msgs
    for i in range(3):
        assert stego_decode(res[i], ecc="none", quality=q, seed_text=seeds[i], lm=lm) == msgs[i]
