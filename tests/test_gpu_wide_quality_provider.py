"""GPU: ``encode_batch`` / ``decode_batch`` / ``stego_encode_batch`` with ``qualities=`` whose top-k is beyond the
single-pass limit -- the api default (top-k 50,000) and the message->bits mode (top-k 60,000, precision 40) among
them.  Such messages run as ONE mixed batch on the wide kernels (``ns_set_stream_quality_wide``); before, every
distinct quality beyond the limit was a call of its own.

A tiny native model whose vocabulary reaches the wide kernel: 2,000 ids, fp16 logits, so K = 1,998 valid ids > 512.
Every comparison is exact against the message alone with its own quality (the one-quality path); the statistics keep
the project's bound (rel 2e-5, abs 2e-6).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

VOCAB = 2000
WIDE = [{"temp": 0.8, "precision": 16, "topk": 50000}, {"temp": 1.0, "precision": 16, "topk": 50000},
        {"temp": 1.2, "precision": 16, "topk": 50000}, {"temp": 1.0, "precision": 20, "topk": 1500},
        {"temp": 1.0, "precision": 40, "topk": 60000}]
NARROW = [{"temp": 0.9, "precision": 26, "topk": 300}, {"temp": 0.7, "precision": 16, "topk": 40}]
Q_OF = [0, 1, 2, 3, 4, 1, 3]  # 7 messages, 5 distinct qualities, all beyond the limit
N_BYTES = [4, 12, 7, 9, 5, 11, 8]


def _provider(vocab=VOCAB):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    model = random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=vocab, n_positions=256)
    return HipArithmeticLM(model, None, logits_dtype="f16", compute_dtype=torch.float16)


def _bits(n_bytes, seed0=500):
    return [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(seed0 + s, n)) for s, n in enumerate(n_bytes)]


def _context(n=33, seed=11):
    return np.random.default_rng(seed).integers(0, VOCAB - 1, size=n).tolist()


def _alone(lm, bits, context, qs, **kw):
    return [lm.encode_batch([b], context, quality=q, **kw) for b, q in zip(bits, qs)]


def _round_trips(out, bits):
    return all(o[: len(b)] == b for o, b in zip(out, bits))


@pytest.fixture(scope="module")
def reference():
    """Every message alone with its own quality (the scalar wide path), tokens and statistics, computed once."""
    lm = _provider()
    assert lm._single_pass_limit() == 512 and lm.mix_wide_qualities
    context = _context()
    bits = _bits(N_BYTES)
    qs = [WIDE[i] for i in Q_OF]
    ref = _alone(lm, bits, context, qs, return_stats=True)
    toks, stats = [r[0][0] for r in ref], [r[1][0] for r in ref]
    under_one = lm.encode_batch(bits, context, quality=qs[1])
    assert sum(a != b for a, b in zip(under_one, toks)) >= 4, "the api default for all gives the same tokens"
    lm.drain_states()
    lm._decode_states.clear()
    return lm, context, bits, qs, toks, stats


def test_wide_qualities_run_as_one_batch_and_equal_each_message_alone(reference):
    lm, context, bits, qs, ref, _ = reference
    got = lm.encode_batch(bits, context, qualities=qs, slots=3)  # 7 messages, 3 slots: refills
    sched = dict(lm.last_schedule)
    assert got == ref
    assert sched["quality_groups"] == 1 and sched["slots"] == 3  # five calls before
    out = lm.decode_batch(got, context, qualities=qs, slots=3)
    assert lm.last_decode_schedule["quality_groups"] == 1
    assert _round_trips(out, bits)
    for m in range(len(bits)):  # the receiver's side: each message alone with its own quality
        alone = lm.decode_batch([got[m]], context, quality=qs[m])[0]
        assert alone[: len(bits[m])] == bits[m], m


def _with_narrow(qs):
    """Messages 5 and 6 take single-pass qualities: all five wide qualities stay, two narrow ones join."""
    qs2 = list(qs)
    qs2[5], qs2[6] = NARROW
    return qs2


def test_narrow_and_wide_messages_make_two_groups_in_the_callers_order(reference):
    lm, context, bits, qs, ref, ref_stats = reference
    qs2 = _with_narrow(qs)
    ref2, stats2 = list(ref), list(ref_stats)
    for m in (5, 6):
        t, s = lm.encode_batch([bits[m]], context, quality=qs2[m], return_stats=True)
        ref2[m], stats2[m] = t[0], s[0]
    lm.drain_states()
    lm._decode_states.clear()
    got, stats = lm.encode_batch(bits, context, qualities=qs2, slots=3, return_stats=True)
    assert got == ref2 and lm.last_schedule["quality_groups"] == 2
    for m in range(len(bits)):
        for k, v in stats2[m].items():
            assert stats[m][k] == pytest.approx(v, rel=2e-5, abs=2e-6), (m, k)
    want = [len(x).to_bytes(8, "big") for x in bits]
    assert [s["residual_bits"] for s in lm.drain_states()] == want
    assert [s["residual_bits"] for s in lm._decode_states] == want
    lm._decode_states.clear()
    out = lm.decode_batch(got, context, qualities=qs2, slots=3)
    assert lm.last_decode_schedule["quality_groups"] == 2
    assert _round_trips(out, bits)
    # the switch off: one call per distinct quality beyond the limit, the same tokens
    lm.mix_wide_qualities = False
    try:
        assert lm.encode_batch(bits, context, qualities=qs2, slots=3) == ref2
        assert lm.last_schedule["quality_groups"] == 1 + 5
        assert _round_trips(lm.decode_batch(got, context, qualities=qs2, slots=3), bits)
        assert lm.last_decode_schedule["quality_groups"] == 1 + 5
    finally:
        del lm.mix_wide_qualities  # back to the class default
    assert lm.mix_wide_qualities


def test_compaction_permutes_the_wide_table(reference):
    lm, context, _, qs, _, _ = reference
    bits = _bits([3, 3, 40, 3, 3, 3, 36], seed0=640)  # two long messages outlive the others: 7 slots -> 2
    ref = [r[0] for r in _alone(lm, bits, context, qs)]
    got = lm.encode_batch(bits, context, qualities=qs)
    assert lm.last_schedule["compactions"] > 0 and lm.last_schedule["quality_groups"] == 1, lm.last_schedule
    assert got == ref
    out = lm.decode_batch(got, context, qualities=qs)
    assert lm.last_decode_schedule["compactions"] > 0, lm.last_decode_schedule
    assert _round_trips(out, bits)


def test_wide_qualities_compose_with_contexts_and_chunked_decode(reference):
    lm, context, bits, qs, ref, _ = reference
    ctxs = [_context(n, seed=20 + n) for n in (1, 31, 32, 33, 64, 65, 100)]
    want = [lm.encode_batch([b], c, quality=q)[0] for b, c, q in zip(bits, ctxs, qs)]
    got = lm.encode_batch(bits, contexts=ctxs, qualities=qs, slots=3)
    assert got == want and lm.last_schedule["quality_groups"] == 1
    out = lm.decode_batch(got, contexts=ctxs, qualities=qs, slots=3)
    assert _round_trips(out, bits)
    one = lm.decode_batch(ref, context, qualities=qs)
    chunked = lm.decode_batch(ref, context, qualities=qs, chunk=4)
    assert lm.last_decode_schedule["chunk"] == 4 and lm.last_decode_schedule["quality_groups"] == 1
    assert chunked == one and _round_trips(chunked, bits)


def test_stego_batch_with_api_default_qualities_is_one_batch():
    from neuralsteganography_amd.stego import stego_decode, stego_decode_batch, stego_encode_batch

    lm = _provider()  # ByteTokenizer over the 2,000-id vocabulary
    # no top-k given: the api default (50,000, beyond the limit); the messages differ in temperature or precision
    qs = [{"temperature": 0.8, "finish_sent": False}, {"precision": 20, "finish_sent": False},
          {"temperature": 1.2, "finish_sent": False}]
    msgs = [b"the api default, message one", bytes(range(30)), b"a third message, warmer than the others"]
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", qualities=qs, seed_text="Dear Alice, ", lm=lm)
    assert [len(r) for r in res] == [2, 2, 2] and lm.last_schedule["quality_groups"] == 1
    assert stego_decode_batch(res, ecc="none", qualities=qs, seed_text="Dear Alice, ", lm=lm) == msgs
    assert lm.last_decode_schedule["quality_groups"] == 1
    for i in range(3):  # each message alone with its own quality, as the reference's receiver decodes it
        assert stego_decode(res[i], ecc="none", quality=qs[i], seed_text="Dear Alice, ", lm=lm) == msgs[i]


def test_a_vocabulary_within_the_single_pass_limit_takes_one_single_pass_batch():
    """512 ids, 510 valid: top-k 50,000 is beyond the limit as a number, but K = min(top-k, valid ids) is not, so the
    coder context has no wide buffers and the single-pass kernel serves the table -- as it served each message's
    scalar call before."""
    from neuralsteganography_amd.stego import stego_decode, stego_decode_batch, stego_encode_batch

    lm = _provider(vocab=512)
    assert lm._single_pass_limit() == 512
    context = np.random.default_rng(11).integers(0, 511, size=33).tolist()
    bits = _bits([6, 9, 5, 8])
    qs = [{"temp": 0.8, "precision": 16, "topk": 50000}, {"temp": 1.0, "precision": 16, "topk": 50000},
          {"temp": 1.2, "precision": 16, "topk": 50000}, {"temp": 1.0, "precision": 40, "topk": 60000}]
    ref = [r[0] for r in _alone(lm, bits, context, qs)]
    got = lm.encode_batch(bits, context, qualities=qs, slots=3)
    assert got == ref and lm.last_schedule["quality_groups"] == 1
    out = lm.decode_batch(got, context, qualities=qs, slots=3)
    assert lm.last_decode_schedule["quality_groups"] == 1 and _round_trips(out, bits)
    mixed = [dict(qs[0]), {"temp": 0.9, "precision": 26, "topk": 300}, dict(qs[2])]  # narrow and "wide" numbers
    narrow_alone = lm.encode_batch([bits[1]], context, quality=mixed[1])[0]
    assert lm.encode_batch(bits[:3], context, qualities=mixed) == [ref[0], narrow_alone, ref[2]]
    assert lm.last_schedule["quality_groups"] == 2
    sq = [{"temperature": 0.8, "finish_sent": False}, {"temperature": 1.2, "finish_sent": False}]  # the api default
    msgs = [b"two messages at the api default", b"that differ in temperature only"]
    res = stego_encode_batch(msgs, chunk_bytes=24, ecc="none", qualities=sq, seed_text="Dear Alice, ", lm=lm)
    assert lm.last_schedule["quality_groups"] == 1
    assert stego_decode_batch(res, ecc="none", qualities=sq, seed_text="Dear Alice, ", lm=lm) == msgs
    for i in range(2):
        assert stego_decode(res[i], ecc="none", quality=sq[i], seed_text="Dear Alice, ", lm=lm) == msgs[i]
