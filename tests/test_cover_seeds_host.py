"""CPU: one seed per message through cover generation and reveal (MockLM, deterministic msg_id).

``cover_generate_batch(secrets, seed_texts=...)`` must equal the per-secret ``cover_generate`` calls, with the gate
off and with the default fallback guard rejecting some messages at attempt 1; ``cover_reveal_batch(texts,
seed_texts=...)`` must return the secrets; the seed arguments are validated; ``return_attempts`` names the attempt
that was accepted.  With the fallback scorer a text's perplexity is its number of distinct whitespace tokens (all
distinct here), so ``max_ppl`` between two seeds' word counts decides which messages go on to a pool seed."""

import pytest

from neuralsteganography_amd import cover, stego
from neuralsteganography_amd.exceptions import ConfigurationError, QualityGateError
from neuralsteganography_amd.lm.mock import MockLM

SECRETS = [b"alpha", "beta beta", b"gamma gamma gamma", b"d", bytes(range(32, 127)) * 2]
SEEDS = ["one two three. ", "x y ", "one two three. ", "the quick brown fox jumps. ", "a longer seed of seven words here. "]
KW = dict(ecc="none", chunk_bytes=40)


@pytest.fixture(autouse=True)
def fixed_msg_id(monkeypatch):
    monkeypatch.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")


def _single(secret, seed, **kw):
    try:
        return cover.cover_generate(secret, seed_text=seed, lm=MockLM(), **KW, **kw)
    except QualityGateError as exc:
        return exc


def _plain(o):
    return o if isinstance(o, str) else (type(o), o.cover_text, o.reasons, o.metrics)


def test_gate_off_equals_per_secret_calls():
    got = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=MockLM(), quality_gate=False, **KW)
    assert got == [_single(s, seed, quality_gate=False) for s, seed in zip(SECRETS, SEEDS)]
    assert all(t.startswith(seed) for t, seed in zip(got, SEEDS))
    assert len(set(got)) == len(got)


@pytest.mark.parametrize("pool, attempts", [(["p q. "], 2), (["a b c d e f g h i. "], 2), ([], 1)])
def test_gate_on_equals_per_secret_calls(pool, attempts):
    """max_ppl 4.5: the 3- and 4-word covers pass at attempt 1, the 6- and 8-word ones go on -- to the pool seed
    (3 words: pass; 10 words: reject), then, the pool being empty, to their own seed again (reject: error)."""
    gate = dict(gate_thresholds={"max_ppl": 4.5}, regen_attempts=attempts, regen_strategy={"seed_pool": pool})
    got = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=MockLM(), return_errors=True, **KW, **gate)
    want = [_single(s, seed, **gate) for s, seed in zip(SECRETS, SEEDS)]
    assert [_plain(o) for o in got] == [_plain(o) for o in want]
    assert [isinstance(o, str) for o in got][:3] == [True] * 3
    if pool == ["p q. "]:
        assert all(isinstance(o, str) for o in got) and got[3].startswith("p q. ") and got[4].startswith("p q. ")
    else:  # rejected everywhere: the error carries the LAST attempt's text, which used the message's own seed
        assert all(isinstance(o, QualityGateError) for o in got[3:])
        assert [o.cover_text.startswith(seed) for o, seed in zip(got[3:], SEEDS[3:])] == [True, True]
        with pytest.raises(QualityGateError) as ei:
            cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=MockLM(), **KW, **gate)
        assert ei.value.cover_text == got[3].cover_text  # the first failing message, in input order


def test_return_attempts_names_the_accepted_attempt():
    gate = dict(gate_thresholds={"max_ppl": 4.5}, regen_attempts=2, regen_strategy={"seed_pool": ["p q. "]})
    got = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=MockLM(), return_attempts=True, **KW, **gate)
    assert [a.seed_variant for _, a in got] == ["base", "base", "base", "alt-1", "alt-1"]
    assert [a.seed_text for _, a in got] == SEEDS[:3] + ["p q. ", "p q. "]
    assert all(t.startswith(a.seed_text) for t, a in got)
    # the receiver reveals every cover with the seed of the attempt that was accepted
    back = cover.cover_reveal_batch([t for t, _ in got], seed_texts=[a.seed_text for _, a in got], lm=MockLM(),
                                    ecc="none")
    assert back == [s.encode() if isinstance(s, str) else s for s in SECRETS]
    off = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=MockLM(), quality_gate=False,
                                     return_attempts=True, **KW)
    assert [(a.seed_text, a.seed_variant) for _, a in off] == [(s, "base") for s in SEEDS]


def test_reveal_with_per_text_seeds():
    lm = MockLM()
    texts = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=lm, quality_gate=False, **KW)
    want = [s.encode() if isinstance(s, str) else s for s in SECRETS]
    assert cover.cover_reveal_batch(texts, seed_texts=SEEDS, ecc="none", lm=lm) == want
    spans = cover.texts_to_spans(texts, seed_texts=SEEDS, lm=lm)
    assert [len(s) for s in spans] == [1, 1, 1, 1, 5]  # 190 bytes in 40-byte chunks
    assert spans == [cover.texts_to_spans([t], seed_text=seed, lm=lm)[0] for t, seed in zip(texts, SEEDS)]
    # a text revealed with another message's seed does not start with it
    from neuralsteganography_amd.codec.errors import DecodeDivergenceError

    with pytest.raises(DecodeDivergenceError):
        cover.cover_reveal_batch(texts, seed_texts=SEEDS[::-1], ecc="none", lm=lm)
    # the shared form is unchanged
    same = cover.cover_generate_batch(SECRETS, seed_text="A seed. ", lm=lm, quality_gate=False, **KW)
    assert cover.cover_reveal_batch(same, seed_text="A seed. ", ecc="none", lm=lm) == want


def test_seed_arguments_are_validated():
    lm = MockLM()
    texts = cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=lm, quality_gate=False, **KW)
    for fn, items in ((cover.cover_generate_batch, SECRETS), (cover.cover_reveal_batch, texts)):
        with pytest.raises(ConfigurationError, match="exactly one"):
            fn(items, lm=lm, ecc="none")
        with pytest.raises(ConfigurationError, match="exactly one"):
            fn(items, seed_text="s", seed_texts=SEEDS, lm=lm, ecc="none")
        with pytest.raises(ConfigurationError, match="4 seed texts for 5 messages"):
            fn(items, seed_texts=SEEDS[:4], lm=lm, ecc="none")
    with pytest.raises(ConfigurationError, match="exactly one"):
        cover.texts_to_spans(texts, lm=lm)
    with pytest.raises(ConfigurationError, match="6 seed texts for 5 messages"):
        cover.texts_to_spans(texts, seed_texts=SEEDS + ["z "], lm=lm)
