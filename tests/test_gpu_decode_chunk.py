"""GPU: ``decode_batch(..., chunk=C)`` / ``stego_decode_batch(..., chunk=C)`` -- a slot's next C cover tokens through
the LM in one forward, the coder token by token -- must decode the SAME BITS as ``chunk=1`` and give the payloads
back, through slot refill, compaction, per-message contexts (equal ones and a shared 64-token prefix), per-message
qualities, fp8 pages, alone after a batched encode, and report a diverging cover for the same message.  On a capped
page pool the decoder (``chunk`` 1 and 5) evicts and re-decodes messages to the same bits, and raises
``KVCapacityError`` for a message that cannot fit alone.

The tiny model of tests/test_gpu_step_chunk.py (n_embd 128, 2 heads, 2 layers, n_positions 64, vocab 512).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import synthetic  # noqa: E402
from neuralsteganography_amd.codec.errors import DecodeDivergenceError  # noqa: E402
from neuralsteganography_amd.exceptions import KVCapacityError  # noqa: E402
from neuralsteganography_amd.lm.kvpages import PAGE_ROWS  # noqa: E402

pytestmark = pytest.mark.gpu

V = 512
Q = {"temp": 0.9, "precision": 26, "topk": 300}
Q2 = {"temp": 0.7, "precision": 16, "topk": 40}
NBYTES = [8, 40, 13, 22, 9, 31, 17, 36, 11, 27, 15, 38]  # 12 messages
CHUNKS = [2, 5, 16]


def _provider(**kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    hf = random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=V, n_positions=64)
    return HipArithmeticLM(hf, None, logits_dtype="f16", compute_dtype=torch.float16, **kw)


def _bits(n_bytes, seed0=900):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _context(n=21, seed=3):
    return np.random.default_rng(seed).integers(0, V - 1, size=n).tolist()


def _check(out, bits):
    assert all(o[: len(b)] == b for o, b in zip(out, bits))


@pytest.fixture(scope="module")
def shared():
    """One shared context, 12 messages encoded in one batch, decoded once with chunk=1 (the reference bits)."""
    lm = _provider()
    bits, context = _bits(NBYTES), _context()
    covers = lm.encode_batch(bits, context, quality=Q)
    assert any(len(c) % C for c in covers for C in CHUNKS)  # token counts that are no multiples of C
    ref = lm.decode_batch(covers, context, quality=Q, slots=4)
    _check(ref, bits)
    return lm, bits, context, covers, ref


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("graphs", [True, False])
def test_chunked_decode_equals_one_token_decode(shared, C, graphs):
    lm, bits, context, covers, ref = shared
    out = lm.decode_batch(covers, context, quality=Q, slots=4 * C, chunk=C, graphs=graphs)  # 4 slots: refills
    sched = dict(lm.last_decode_schedule)
    assert out == ref
    _check(out, bits)
    assert sched["slots"] == 4 and sched["chunk"] == C  # 12 messages through 4 slots: every slot is refilled


@pytest.mark.parametrize("C", CHUNKS)
def test_compaction_moves_the_carried_rows(shared, C):
    """Two long messages outlive five short ones: the 7 slots are compacted to the live ones, whose carried logits
    rows, states and page tables move with them."""
    lm, _, context, _, _ = shared
    bits = _bits([3, 3, 40, 3, 3, 3, 36], seed0=640)
    covers = lm.encode_batch(bits, context, quality=Q)
    ref = lm.decode_batch(covers, context, quality=Q)
    out = lm.decode_batch(covers, context, quality=Q, slots=7 * C, chunk=C)
    assert lm.last_decode_schedule["slots"] == 7 and lm.last_decode_schedule["compactions"] > 0
    assert out == ref
    _check(out, bits)


def test_slot_rule_divides_the_callers_slots(shared):
    lm, bits, context, covers, ref = shared
    out = lm.decode_batch(covers, context, quality=Q, slots=10, chunk=5)
    assert lm.last_decode_schedule["slots"] == 2 and out == ref
    out = lm.decode_batch(covers, context, quality=Q, slots=3, chunk=16)  # fewer slots than the chunk: one slot
    assert lm.last_decode_schedule["slots"] == 1 and out == ref


@pytest.mark.parametrize("C", CHUNKS)
def test_chunked_decode_with_contexts_and_qualities(C):
    """Two messages with equal contexts, two sharing a 64-token prefix, two distinct qualities."""
    lm = _provider()
    rng = np.random.default_rng(17)
    head = rng.integers(0, V - 1, size=64).tolist()
    same = rng.integers(0, V - 1, size=37).tolist()
    ctxs = [rng.integers(0, V - 1, size=int(n)).tolist() for n in rng.integers(5, 90, size=len(NBYTES))]
    ctxs[1], ctxs[6] = same, list(same)
    ctxs[3], ctxs[8] = head + [5, 6, 7], head + [9, 10, 11, 12, 13]
    qs = [Q if m % 3 else Q2 for m in range(len(NBYTES))]
    bits = _bits(NBYTES, seed0=1200)
    covers = lm.encode_batch(bits, contexts=ctxs, qualities=qs)
    ref = lm.decode_batch(covers, contexts=ctxs, qualities=qs, slots=4)
    _check(ref, bits)
    out = lm.decode_batch(covers, contexts=ctxs, qualities=qs, slots=4 * C, chunk=C)
    assert out == ref
    assert lm.last_decode_schedule["prefill_shared"] >= 2


@pytest.mark.parametrize("C", CHUNKS)
def test_chunked_decode_over_fp8_pages(C):
    lm = _provider(kv_dtype="fp8")
    bits, context = _bits(NBYTES, seed0=1500), _context(seed=4)
    covers = lm.encode_batch(bits, context, quality=Q)
    ref = lm.decode_batch(covers, context, quality=Q, slots=4)
    _check(ref, bits)
    assert lm.decode_batch(covers, context, quality=Q, slots=4 * C, chunk=C) == ref


def test_one_message_alone_after_a_batched_encode(shared):
    lm, bits, context, covers, ref = shared
    m = 7
    alone = lm.decode_batch([covers[m]], context, quality=Q, chunk=8)
    assert alone == [ref[m]] and alone[0][: len(bits[m])] == bits[m]


def test_divergence_names_the_same_message(shared):
    """One token of message 5 replaced by an id outside the kept top-k (Q2 keeps 40 of 512): the chunked decode
    raises the error of the one-token decode."""
    lm, _, context, _, _ = shared
    bits = _bits(NBYTES[:8], seed0=1700)
    covers = [list(c) for c in lm.encode_batch(bits, context, quality=Q2)]
    m, pos = 5, 7
    assert len(covers[m]) > pos + 3
    message = None
    for cand in range(V - 1):  # the first replacement the one-token decode rejects
        if cand == covers[m][pos]:
            continue
        broken = [list(c) for c in covers]
        broken[m][pos] = cand
        try:
            lm.decode_batch(broken, context, quality=Q2, slots=4)
        except DecodeDivergenceError as e:
            message = str(e)
            break
    assert message is not None and "[5]" in message
    for C in (2, 16):
        with pytest.raises(DecodeDivergenceError) as ei:
            lm.decode_batch(broken, context, quality=Q2, slots=4 * C, chunk=C)
        assert str(ei.value) == message


def test_stego_decode_batch_takes_chunk():
    from neuralsteganography_amd.stego import stego_decode_batch, stego_encode_batch

    lm = _provider()
    q = dict(Q, finish_sent=False)
    msgs = [b"several tokens per forward, same bits", bytes(range(60))]  # 2 and 3 packets of 24 bytes
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", quality=q, seed_text="Dear Alice, ", lm=lm)
    assert [len(r) for r in res] == [2, 3]
    assert stego_decode_batch(res, ecc="none", quality=q, seed_text="Dear Alice, ", lm=lm, chunk=4) == msgs
    assert lm.last_decode_schedule["chunk"] == 4
    with pytest.raises(ValueError):
        stego_decode_batch(res, ecc="none", quality=q, seed_text="Dear Alice, ", lm=lm, chunk=17)


def test_chunk_is_validated():
    lm = _provider()
    for bad in (0, 17, 2.0, "4", True):
        with pytest.raises(ValueError):
            lm.decode_batch([[1, 2, 3]], _context(), quality=Q, chunk=bad)
    lm.lm.window = 8
    try:
        with pytest.raises(ValueError):
            lm.decode_batch([[1, 2, 3]], _context(), quality=Q, chunk=2)
    finally:
        lm.lm.window = 0


def _capped(cap_pages):
    """A fresh provider whose page pool never holds more than ``cap_pages`` pages."""
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    return lm, pool


@pytest.fixture(scope="module", params=[False, True], ids=["one_context", "contexts"])
def evictable(request):
    """8 messages of 24-40 bytes at Q2 (at most log2(40) bits a token: every cover is longer than one page), encoded
    and decoded on an uncapped pool, and a pool cap under which they cannot all be live at once.  A message's pages at
    its peak are ``ceil(rows / 32)``, its rows the cover's tokens and, with per-message contexts, its context's (the
    one shared context lies outside the pool).  The cap is two pages more than the longest message needs alone: the
    first admission then takes ``cap - 1`` messages at one page each (a context of at most 12 tokens and the first
    20 positions), and they all need their second page at the same check."""
    lm = _provider()
    bits = _bits([40, 24, 36, 28, 32, 26, 38, 30], seed0=2100)
    if request.param:
        rng = np.random.default_rng(23)
        kw = {"contexts": [rng.integers(0, V - 1, size=int(n)).tolist() for n in rng.integers(3, 13, size=len(bits))]}
        own = [len(c) for c in kw["contexts"]]
    else:
        kw, own = {"context": _context()}, [0] * len(bits)
    covers = lm.encode_batch(bits, quality=Q2, **kw)
    ref = lm.decode_batch(covers, quality=Q2, **kw)
    _check(ref, bits)
    need = [-(-(t + len(c)) // PAGE_ROWS) for t, c in zip(own, covers)]
    cap_pages = max(need) + 2
    assert max(need) <= cap_pages < sum(need), (need, cap_pages)
    return covers, kw, ref, cap_pages


@pytest.mark.parametrize("C", [1, 5])
def test_decoder_evicts_when_the_pool_is_small_and_gives_the_same_bits(evictable, C):
    covers, kw, ref, cap_pages = evictable
    lm, pool = _capped(cap_pages)
    out = lm.decode_batch(covers, quality=Q2, chunk=C, **kw)
    sched = dict(lm.last_decode_schedule)
    print(f"cap_pages={cap_pages} chunk={C} {sorted(kw)} schedule={sched} pool={pool.free_pages}/{pool.total}")
    assert out == ref
    assert sched["evictions"] > 0, sched
    assert pool.total <= cap_pages
    assert pool.free_pages == pool.total  # every page came back


@pytest.mark.parametrize("C", [1, 5])
def test_decoder_kv_capacity_error_not_torch_oom(C):
    """One cover of more than 64 tokens on a pool of 2 pages (64 positions): ``KVCapacityError``, and the pool never
    grows past its cap.  The failed message still holds its two pages when the error leaves the loop (0 of 2 free,
    measured at both chunks); the next call's ``begin_slots`` frees them."""
    context = _context()
    covers = _provider().encode_batch(_bits([60], seed0=2300), context, quality=Q2)
    assert len(covers[0]) > 2 * PAGE_ROWS
    lm, pool = _capped(2)
    with pytest.raises(KVCapacityError):
        lm.decode_batch(covers, context, quality=Q2, chunk=C)
    print(f"chunk={C} pool={pool.free_pages}/{pool.total}")
    assert pool.total <= 2
