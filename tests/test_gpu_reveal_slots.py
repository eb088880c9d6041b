"""GPU: cover texts revealed as one slot-scheduled batch with one seed and one quality per text
(``HipArithmeticLM.reveal_spans``, ``lm/slots.py`` ``SlotRevealer``, ``texts_to_spans(qualities=, slots=)``,
``cover_reveal_batch(attempts=)``).

The contract: a text's spans are those the existing round-based ``texts_to_spans`` finds for it -- whatever slot it
runs in, whatever its neighbours, through evictions, on the wide kernels, and when the text has to fall back to the
BPE repair.  Every comparison is exact (token id lists, secrets, error texts).  The native fp16 tiny model of
``tests/test_gpu_cover_seeds.py`` behind the id-exact tokenizer, ``ecc="none"`` and a fixed ``make_msg_id``.
"""

import numpy as np
import pytest
from test_gpu_cover_seeds import CharMergeTokenizer, IdTokenizer

from neuralsteganography_amd import stego, synthetic
from neuralsteganography_amd.codec.errors import DecodeDivergenceError
from neuralsteganography_amd.exceptions import KVCapacityError

pytestmark = pytest.mark.gpu

V = 2000
BASE = {"temp": 0.9, "precision": 26, "topk": 300}
OVERRIDES = [{}, {"top_k": 80, "temp": 0.8}, {"top_k": 70, "temp": 0.7}]  # the regeneration schedule's first steps
N = 12
SECRETS = [synthetic.payload_bytes(70 + i, 49 + i) for i in range(N)]  # 49..60 bytes: three 24-byte chunks each
SEED_OF = [i % 4 for i in range(N)]
# four (seed, quality) pairs over the 12 texts: every seed and every quality occurs, three texts per pair
Q_OF = [(i % 4) % 3 for i in range(N)]


@pytest.fixture(autouse=True)
def fixed_msg_id(monkeypatch):
    monkeypatch.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")


def _provider(cap_pages=None):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    m = random_gpt2("tiny", vocab_size=V, n_positions=1024, n_embd=128, n_head=2, seed=23)
    lm = HipArithmeticLM(m, IdTokenizer(V))
    assert lm.lm.native
    if cap_pages is None:
        return lm
    lm.lm.kv_segment_pages = 1  # a page-exact budget, as tests/test_gpu_decode_chunk.py caps its pool
    pool = lm.lm.page_pool()
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    return lm, pool


def _seeds():
    """Four seeds: two equal (33 ids), two that share a 64-id head (70 and 97 ids)."""
    tok = IdTokenizer(V)
    rng = np.random.default_rng(3)
    ids = lambda n: [int(t) for t in rng.integers(4, V - 1, size=n) if t != 628]  # noqa: E731
    a, head = ids(33), ids(64)
    return [tok.decode(a).strip(), tok.decode(a).strip(), tok.decode(head + ids(6)).strip(),
            tok.decode(head + ids(33)).strip()]


@pytest.fixture(scope="module")
def lm():
    return _provider()


_CASES = {}


def _case(lm, finish_sent):
    """The 12 covers (generated per quality, as attempt r of ``cover_generate_batch`` generates them), and the spans
    the existing ``texts_to_spans`` finds for them, called once per distinct (seed, quality).  Computed once per
    ``finish_sent`` and shared."""
    from neuralsteganography_amd import cover

    if finish_sent in _CASES:
        return _CASES[finish_sent]
    mp = pytest.MonkeyPatch()
    mp.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")
    try:
        base = dict(BASE, finish_sent=finish_sent)
        four = _seeds()
        seeds = [four[s] for s in SEED_OF]
        qs = [{**stego.normalise_quality(base), **OVERRIDES[k]} for k in Q_OF]
        texts = [None] * N
        for k in range(3):
            members = [i for i in range(N) if Q_OF[i] == k]
            got = cover.cover_generate_batch([SECRETS[i] for i in members], seed_texts=[seeds[i] for i in members],
                                             quality=qs[members[0]], ecc="none", chunk_bytes=24, quality_gate=False,
                                             lm=lm)
            for i, t in zip(members, got):
                texts[i] = t
        want = [None] * N
        for pair in sorted({(seeds[i], Q_OF[i]) for i in range(N)}):
            members = [i for i in range(N) if (seeds[i], Q_OF[i]) == pair]
            res = cover.texts_to_spans([texts[i] for i in members], seed_text=pair[0], quality=qs[members[0]], lm=lm)
            for i, sp in zip(members, res):
                want[i] = sp
    finally:
        mp.undo()
    assert all(len(sp) == 3 for sp in want), [len(sp) for sp in want]
    _CASES[finish_sent] = (base, seeds, qs, texts, want)
    return _CASES[finish_sent]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "finish_sent"])
def case(request, lm):
    return _case(lm, request.param)


@pytest.fixture(scope="module")
def plain(lm):
    return _case(lm, False)


def test_spans_and_secrets_in_one_slot_batch(case, lm):
    from neuralsteganography_amd import cover

    base, seeds, qs, texts, want = case
    got = cover.texts_to_spans(texts, qualities=qs, seed_texts=seeds, slots=4, lm=lm)
    sched = dict(lm.last_reveal_schedule)
    print("schedule", sched, "tokens", sum(len(s) for sp in want for s in sp))
    for i in range(N):
        assert got[i] == want[i], f"text {i}"
    # an id-exact tokenizer never diverges: the batch did not pass by sending every text down the round-based path
    assert sched["fallback_texts"] == 0
    assert sched["spans"] == sum(len(sp) for sp in want) == 3 * N
    assert sched["quality_groups"] == 1 and sched["steps"] > 0 and sched["prefill_rows"] > 0
    attempts = [cover.Attempt(seeds[i], OVERRIDES[Q_OF[i]], "base" if Q_OF[i] == 0 else f"alt-{Q_OF[i]}")
                for i in range(N)]
    assert cover.cover_reveal_batch(texts, attempts=attempts, quality=base, ecc="none", lm=lm) == SECRETS
    assert lm.last_reveal_schedule["fallback_texts"] == 0


def test_a_small_pool_evicts_and_gives_the_same_spans(plain):
    from neuralsteganography_amd import cover
    from neuralsteganography_amd.lm.kvpages import PAGE_ROWS

    base, seeds, qs, texts, want = plain
    tok = IdTokenizer(V)
    need = [-(-(1 + len(tok.encode(t))) // PAGE_ROWS) for t in texts]  # <|endoftext|>, the seed's and the cover's ids
    cap_pages = max(need) + 2
    assert max(need) <= cap_pages < sum(need), (need, cap_pages)
    capped, pool = _provider(cap_pages)
    got = cover.texts_to_spans(texts, qualities=qs, seed_texts=seeds, slots=N, lm=capped)
    sched = dict(capped.last_reveal_schedule)
    print(f"cap_pages={cap_pages} schedule={sched} pool={pool.free_pages}/{pool.total}")
    assert got == want
    assert sched["evictions"] > 0 and sched["fallback_texts"] == 0, sched
    assert sched["kv_pages_peak"] <= cap_pages and pool.total <= cap_pages
    assert pool.free_pages == pool.total  # every page came back


@pytest.mark.parametrize("i", [1, 6])
def test_a_text_alone_equals_itself_in_the_batch(plain, lm, i):
    from neuralsteganography_amd import cover

    base, seeds, qs, texts, want = plain
    assert cover.texts_to_spans([texts[i]], qualities=[qs[i]], seed_texts=[seeds[i]], slots=1, lm=lm) == [want[i]]
    assert lm.last_reveal_schedule["fallback_texts"] == 0 and lm.last_reveal_schedule["spans"] == 3


def test_wide_group_next_to_a_single_pass_group(lm):
    """Half the texts at the api default top-k 50,000 (1,998 valid ids: the wide chain), half at top-k 300."""
    from neuralsteganography_amd import cover

    wide = {"temp": 1.0, "precision": 26, "topk": 50000, "finish_sent": False}
    narrow = dict(BASE, finish_sent=False)
    four = _seeds()
    secrets = [synthetic.payload_bytes(300 + i, 25 + i) for i in range(4)]  # two 24-byte chunks each
    seeds = [four[0], four[2], four[3], four[1]]
    qs = [wide, narrow, wide, narrow]
    texts, want = [None] * 4, [None] * 4
    for q in (wide, narrow):
        members = [i for i in range(4) if qs[i] is q]
        kw = dict(seed_texts=[seeds[i] for i in members], quality=q, lm=lm)
        for i, t in zip(members, cover.cover_generate_batch([secrets[i] for i in members], ecc="none", chunk_bytes=24,
                                                            quality_gate=False, **kw)):
            texts[i] = t
        for i, sp in zip(members, cover.texts_to_spans([texts[i] for i in members], **kw)):
            want[i] = sp
    got = cover.texts_to_spans(texts, qualities=qs, seed_texts=seeds, slots=4, lm=lm)
    sched = dict(lm.last_reveal_schedule)
    assert got == want and all(len(sp) == 2 for sp in got)
    assert sched["quality_groups"] == 2 and sched["fallback_texts"] == 0 and sched["spans"] == 8, sched
    assert cover.cover_reveal_batch(texts, qualities=qs, seed_texts=seeds, ecc="none", lm=lm) == secrets


def test_a_text_that_needs_the_bpe_repair_falls_back():
    """The vocabulary-64 merge tokenizer of test_decode_counted_repair_with_contexts_equals_alone: the re-tokenised
    covers hold merges the coder never emitted, so those texts diverge in their slot, leave the batch and are
    repaired by the round-based path -- every text's spans are that path's, fallen back or not."""
    from neuralsteganography_amd import cover
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    tok = CharMergeTokenizer()
    m = random_gpt2("tiny", vocab_size=64, n_positions=2048, n_embd=128, n_head=2, seed=29)
    lm = HipArithmeticLM(m, tok, banned=tok.banned())
    q = {"temp": 1.0, "precision": 26, "topk": 300, "finish_sent": False}
    long_a, head = "Abc" * 11, "Qrs" * 22
    seeds = [long_a, head + "Xy", long_a, head + "Zw" * 16, head + "Xy", head + "Zw" * 16]
    secrets = [synthetic.payload_bytes(s, 20 + 4 * s) for s in range(6)]
    kw = dict(seed_texts=seeds, quality=q, lm=lm)
    texts = cover.cover_generate_batch(secrets, ecc="none", chunk_bytes=64, quality_gate=False, **kw)
    want = cover.texts_to_spans(texts, **kw)
    got = cover.texts_to_spans(texts, slots=3, **kw)
    sched = dict(lm.last_reveal_schedule)
    print("schedule", sched)
    assert sched["fallback_texts"] >= 1, "no merge in any re-tokenised cover: pick other secrets"
    assert got == want
    assert sched["spans"] == sum(len(sp) for sp in want)
    assert cover.cover_reveal_batch(texts, slots=3, ecc="none", **kw) == secrets


def test_errors_are_those_of_the_round_based_path(plain, lm):
    from neuralsteganography_amd import cover

    base, seeds, qs, texts, want = plain
    tok = IdTokenizer(V)
    i = 2
    cut = tok.decode(tok.encode(texts[i])[: len(tok.encode(seeds[i])) + 30]).strip()  # inside the first packet
    kw = dict(seed_texts=[seeds[i]], lm=lm)
    with pytest.raises(DecodeDivergenceError) as old:
        cover.texts_to_spans([cut], quality=qs[i], **kw)
    with pytest.raises(DecodeDivergenceError) as new:
        cover.texts_to_spans([cut], qualities=[qs[i]], slots=2, **kw)
    assert str(new.value) == str(old.value) and "no complete packet in the remaining 30 tokens" in str(new.value)
    capped, pool = _provider(2)  # two pages hold 64 positions: no cover fits
    with pytest.raises(KVCapacityError):
        cover.texts_to_spans([texts[i]], qualities=[qs[i]], seed_texts=[seeds[i]], slots=1, lm=capped)
