"""GPU: ``finish_sent`` through refilled and evicted slots (``lm/slots.py``; reference:
``code_base/arithmetic.py:114,134-137``, after the payload the top-1 token is emitted until one ends a sentence).

Twelve ragged messages (a 0-bit and a 1-bit one among them) on the native provider with a sentence-end table that
marks most ids -- a random tied-embedding LM falls into greedy fixed points, so with the tokenizer's real table a
tail never ends; with 7 of 8 ids marked it is short and cannot run away.  The same tokens must come out of all
twelve slots at once, of 4 slots with graphs, of 5 eager slots and of a page-exact pool that evicts; the CPU oracle
replays messages from their own logits; decoding through 3 slots recovers every payload; the pool is whole after.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import synthetic  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

Q = {"temp": 0.9, "precision": 26, "topk": 300, "finish_sent": True}
NBITS = [160, 24, 256, 96, 1, 200, 0, 64, 320, 80, 120, 40]  # ragged; message 4 has one bit, message 6 none
REPLAYED = (2, 4, 6)  # replayed alone through the oracle: a long one, the 1-bit and the 0-bit message


def _provider(seed=41, **kw):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    lm = HipArithmeticLM(random_gpt2("gpt2", seed=seed), None, logits_dtype="f16", logit_scale=6.0, **kw)
    lm._sent_end = (np.arange(lm.vocab) % 8 != 3).astype(np.uint8)
    return lm


def _bits():
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(500 + s, (n + 7) // 8))[:n] for s, n in
            enumerate(NBITS)]


def _record_alone(lm, bits, ctx):
    """One message alone through one slot, eager, with every step's logits copied to the host."""
    seen = []
    orig_prefill, orig_static = lm.lm.prefill, lm.lm.step_static

    def rec_prefill(*a, **k):
        out = orig_prefill(*a, **k)
        seen.append(out[0, : lm.vocab].float().cpu().numpy())
        return out

    def rec_static(tok):
        out = orig_static(tok)
        seen.append(out[0, : lm.vocab].float().cpu().numpy())
        return out

    lm.lm.prefill, lm.lm.step_static = rec_prefill, rec_static
    try:
        toks = lm.encode_batch([bits], ctx, quality=Q, graphs=False)[0]
    finally:
        lm.lm.prefill, lm.lm.step_static = orig_prefill, orig_static
    return toks, seen


def test_finish_sent_through_refilled_and_evicted_slots():
    lm = _provider()
    table = lm._sent_end
    ctx = [lm.vocab - 1] + list(synthetic.DEFAULT_CONTEXT[1:])
    bits = _bits()
    assert [len(b) for b in bits] == NBITS
    lock = lm.encode_batch(bits, ctx, quality=Q)  # all 12 slots at once
    assert lm.encode_batch(bits, ctx, quality=Q, slots=4) == lock  # 12 messages through 4 slots, graphs
    assert lm.encode_batch(bits, ctx, quality=Q, slots=5, graphs=False) == lock
    for t in lock:
        assert not t or table[t[-1]]  # every non-empty cover ends on a sentence end
    tails = {}
    for s in REPLAYED:
        alone, seen = _record_alone(lm, bits[s], ctx)
        assert alone == lock[s], s
        o, traces = oracle.encode_stream(lambda t: seen[t], bits[s], banned=[lm.vocab - 1, 628], temp=Q["temp"],
                                         precision=Q["precision"], topk=Q["topk"], sent_end=table)
        assert o == lock[s], s
        tails[s] = len(o) - len(traces)  # the oracle's trace has one entry per step that still fixed payload bits
        assert all(not table[t] for t in o[len(traces):-1]) and table[o[-1]]
    print("finish tails (tokens after the payload's last bit):", tails, "cover lengths:", [len(t) for t in lock])
    assert sum(n > 0 for n in tails.values()) >= 3, tails
    out = lm.decode_batch(lock, ctx, quality=Q, slots=3)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    assert lm.lm.pool.free_pages == lm.lm.pool.total  # every page came back: the pool is whole

    # the same call under a page-exact pool of 14 pages: the youngest messages are evicted and re-queued
    small = _provider()
    small.lm.kv_segment_pages = 1
    pool = small.lm.page_pool()
    cap_pages = 14
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    assert small.encode_batch(bits, ctx, quality=Q) == lock
    assert small.last_schedule["evictions"] > 0, small.last_schedule
    assert pool.total <= cap_pages and pool.free_pages == pool.total
    out = small.decode_batch(lock, ctx, quality=Q, slots=3)
    assert all(o[: len(b)] == b for o, b in zip(out, bits))
    assert pool.free_pages == pool.total
