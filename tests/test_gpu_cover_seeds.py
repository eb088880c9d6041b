"""GPU: one seed per message through the whole cover path -- the counted decodes with ``contexts=``, cover generation
with ``seed_texts=`` (gate off, gate on with the GPU guard, an impossible gate) and reveal from text.  Every batched
result is compared with the same message run alone: the native fp16 model's step, prefill and scoring forward are
batch-invariant, so the tokens, bits and guard metrics must be identical, not close."""

import numpy as np
import pytest
from test_gpu_guard import CharMergeTokenizer, IdTokenizer

from neuralsteganography_amd import stego, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fixed_msg_id(monkeypatch):
    monkeypatch.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")


@pytest.fixture(scope="module")
def provider():
    """The native fp16 tiny model (2 layers, 2 heads of 64) behind the id-exact tokenizer of test_gpu_guard.py."""
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    m = random_gpt2("tiny", vocab_size=2000, n_positions=1024, n_embd=128, n_head=2, seed=23)
    lm = HipArithmeticLM(m, IdTokenizer(2000))
    assert lm.lm.native
    return lm


Q = {"temp": 0.9, "precision": 26, "topk": 300, "finish_sent": False}


def _contexts():
    """6 streams over 3 distinct contexts: two streams with equal contexts (33 tokens: across the 32-row page
    boundary), two whose contexts share a 64-token head (70 and 97 tokens), and each of those once more."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1999, size=33).tolist()
    head = rng.integers(0, 1999, size=64).tolist()
    b = head + rng.integers(0, 1999, size=6).tolist()
    c = head + rng.integers(0, 1999, size=33).tolist()
    return [a, b, a, c, b, c]


def test_decode_counted_with_contexts_equals_alone(provider):
    lm = provider
    ctxs = _contexts()
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 6 + 3 * s)) for s in range(6)]
    toks = lm.encode_batch(bits, contexts=ctxs, quality=Q)
    assert len({len(t) for t in toks}) > 1  # ragged: streams end at different steps
    got_bits, got_counts = lm.decode_counted(toks, contexts=ctxs, quality=Q)
    assert lm.lm.last_prefill["shared"] >= 2 and lm.lm.last_prefill.get("prefix_entries", 0) >= 1  # pages were shared
    for s in range(6):
        b1, c1 = lm.decode_counted([toks[s]], ctxs[s], quality=Q)
        assert got_bits[s] == b1[0] and got_counts[s] == c1[0], s
        assert got_bits[s][: len(bits[s])] == bits[s]
        assert len(got_counts[s]) == len(toks[s]) and got_counts[s][-1] == len(got_bits[s])
    # a stream decoded after another stream's context gives other bits: the contexts are really per stream
    wrong, _ = lm.decode_counted([toks[0]], ctxs[1], quality=Q)
    assert wrong[0][: len(bits[0])] != bits[0]
    from neuralsteganography_amd.exceptions import ConfigurationError

    with pytest.raises(ConfigurationError):
        lm.decode_counted(toks, ctxs[0], contexts=ctxs, quality=Q)
    with pytest.raises(ConfigurationError):
        lm.decode_counted(toks, contexts=ctxs[:5], quality=Q)


def test_decode_counted_repair_with_contexts_equals_alone():
    """The vocabulary-64 merge tokenizer of test_cover_text_reveal_with_bpe_repair: the re-tokenised covers hold
    merges the coder never emitted, so the repair edits the lists -- identically in the batch and alone."""
    from neuralsteganography_amd.codec.textio import seed_to_ids, spans_to_text
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2
    from neuralsteganography_amd.stego import stego_encode_batch

    tok = CharMergeTokenizer()
    m = random_gpt2("tiny", vocab_size=64, n_positions=2048, n_embd=128, n_head=2, seed=29)
    lm = HipArithmeticLM(m, tok, banned=tok.banned())
    q = {"temp": 1.0, "precision": 26, "topk": 300, "finish_sent": False}
    long_a, head = "Abc" * 11, "Qrs" * 22  # 33 ids; a 66-id head whose first 64 ids are shared
    seeds = [long_a, head + "Xy", long_a, head + "Zw" * 16, head + "Xy", head + "Zw" * 16]
    secrets = [synthetic.payload_bytes(s, 20 + 4 * s) for s in range(6)]
    res = stego_encode_batch(secrets, chunk_bytes=64, ecc="none", quality=q, seed_texts=seeds, lm=lm)
    lists, ctxs = [], []
    for r, seed in zip(res, seeds):
        seed_ids = seed_to_ids(seed, tok)
        ids = tok.encode(spans_to_text([list(s) for s in r], seed_ids, tok))
        assert ids[: len(seed_ids)] == seed_ids
        lists.append(ids[len(seed_ids):])
        ctxs.append(lm.encode_seed(seed))
    bits, counts, fixed, edits = lm.decode_counted_repair(lists, contexts=ctxs, quality=q)
    assert sum(len(e) for e in edits) >= 1, "no merge in any re-tokenised cover: pick other secrets"
    for s in range(6):
        b1, c1, f1, e1 = lm.decode_counted_repair([lists[s]], ctxs[s], quality=q)
        assert (bits[s], counts[s], fixed[s], edits[s]) == (b1[0], c1[0], f1[0], e1[0]), s
    assert lm.decode_tokens_repair(lists, contexts=ctxs, quality=q) == bits


SEEDS = ["w5. w6. w3", "w7. w8. w9. w10", "w5. w6. w3", "w11", "w7. w8. w12. w13. w14"]
SECRETS = [b"first secret", bytes(range(40)), b"z", b"the fourth one", b"5five"]
POOL = {"seed_pool": ["w20. w21", "w22. w23. w24"], "top_k_steps": [], "temperature_steps": []}
OPEN_GATE = {"max_ppl": 1e12, "max_ngram_repeat": 1.0, "min_ttr": 0.0, "max_avg_entropy": 1e9}


def _guard(lm):
    from neuralsteganography_amd.detect import QualityGuard
    from neuralsteganography_amd.metrics import HipLMScorer, LMScorer

    return QualityGuard(lm_scorer=LMScorer(scorer=HipLMScorer.from_provider(lm)))


def test_cover_generate_batch_with_seed_texts(provider):
    from neuralsteganography_amd.cover import cover_generate, cover_generate_batch
    from neuralsteganography_amd.exceptions import QualityGateError

    lm = provider
    kw = dict(quality=Q, ecc="none", lm=lm, chunk_bytes=24)
    # gate off
    alone = [cover_generate(s, seed_text=seed, quality_gate=False, **kw) for s, seed in zip(SECRETS, SEEDS)]
    assert cover_generate_batch(SECRETS, seed_texts=SEEDS, quality_gate=False, **kw) == alone
    assert all(t.startswith(seed) for t, seed in zip(alone, SEEDS))
    # gate on: max_ppl between the attempt-1 perplexities of the per-secret path, so some covers pass at once and
    # the others go on to the pool seeds
    guard = _guard(lm)
    ppl = sorted(v.metrics["ppl"] for v in guard.evaluate_batch(alone, OPEN_GATE))
    assert ppl[1] < ppl[2]
    gate = dict(gate_thresholds=dict(OPEN_GATE, max_ppl=0.5 * (ppl[1] + ppl[2])), regen_attempts=2, regen_strategy=POOL,
                quality_guard=guard)
    want = []
    for s, seed in zip(SECRETS, SEEDS):
        try:
            want.append(cover_generate(s, seed_text=seed, **kw, **gate))
        except QualityGateError as exc:
            want.append(exc)
    got = cover_generate_batch(SECRETS, seed_texts=SEEDS, return_errors=True, return_attempts=True, **kw, **gate)
    variants = []
    for g, w in zip(got, want):
        if isinstance(w, QualityGateError):
            assert isinstance(g, QualityGateError)
            assert (g.cover_text, g.reasons, g.metrics) == (w.cover_text, w.reasons, w.metrics)
            variants.append("rejected")
        else:
            assert g[0] == w and g[0].startswith(g[1].seed_text)
            variants.append(g[1].seed_variant)
    assert variants.count("base") == 2, variants  # passed at attempt 1 ...
    assert len([v for v in variants if v != "base"]) == 3, variants  # ... and went on to a pool seed
    # an impossible gate: one error per message, each equal to the per-secret path's
    hard = dict(gate, gate_thresholds={"max_ppl": 0.5})
    errs = cover_generate_batch(SECRETS[:3], seed_texts=SEEDS[:3], return_errors=True, **kw, **hard)
    assert all(isinstance(e, QualityGateError) and e.reasons[0].startswith("ppl ") for e in errs)
    with pytest.raises(QualityGateError) as ei:
        cover_generate(SECRETS[1], seed_text=SEEDS[1], **kw, **hard)
    assert (errs[1].cover_text, errs[1].metrics) == (ei.value.cover_text, ei.value.metrics)


@pytest.mark.parametrize("finish_sent", [False, True])
def test_cover_reveal_batch_with_seed_texts(provider, finish_sent):
    from neuralsteganography_amd.cover import cover_generate_batch, cover_reveal, cover_reveal_batch

    lm = provider
    q = dict(Q, finish_sent=finish_sent)
    kw = dict(quality=q, ecc="none", lm=lm)
    texts = cover_generate_batch(SECRETS, seed_texts=SEEDS, quality_gate=False, chunk_bytes=24, **kw)
    assert cover_reveal_batch(texts, seed_texts=SEEDS, **kw) == SECRETS
    assert cover_reveal(texts[1], seed_text=SEEDS[1], **kw) == SECRETS[1]


def test_reveal_covers_accepted_at_a_later_attempt(provider):
    from neuralsteganography_amd.cover import cover_generate_batch, cover_reveal_batch

    lm = provider
    kw = dict(quality=Q, ecc="none", lm=lm)
    guard = _guard(lm)
    first = cover_generate_batch(SECRETS, seed_texts=SEEDS, quality_gate=False, chunk_bytes=24, **kw)
    ppl = sorted(v.metrics["ppl"] for v in guard.evaluate_batch(first, OPEN_GATE))
    # four pool seeds for the three covers above the threshold; whatever passes is revealed with its attempt's seed
    pool = dict(POOL, seed_pool=POOL["seed_pool"] + ["w25. w26", "w27"])
    got = cover_generate_batch(SECRETS, seed_texts=SEEDS, chunk_bytes=24, return_errors=True, return_attempts=True,
                               gate_thresholds=dict(OPEN_GATE, max_ppl=0.5 * (ppl[1] + ppl[2])), regen_attempts=4,
                               regen_strategy=pool, quality_guard=guard, **kw)
    ok = [i for i, g in enumerate(got) if isinstance(g, tuple)]
    later = [i for i in ok if got[i][1].seed_variant != "base"]
    assert later, [g[1].seed_variant if isinstance(g, tuple) else "rejected" for g in got]
    assert all(got[i][1].seed_text in pool["seed_pool"] for i in later)
    back = cover_reveal_batch([got[i][0] for i in ok], seed_texts=[got[i][1].seed_text for i in ok], **kw)
    assert back == [SECRETS[i] for i in ok]
