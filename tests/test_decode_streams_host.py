"""CPU: the host side of the per-text reveal (library 0.31.6) -- the ``ns_decode_step_streams`` binding against the
header, its refusals that need no device, and ``qualities=`` / ``attempts=`` / ``slots=`` of the cover front end on
the mock provider, where they are served by one existing call per distinct quality.

The kernel entry itself is in ``tests/test_gpu_decode_streams.py`` (every refused argument on a live context
included: a context cannot be created without a GPU), the slot scheduler in ``tests/test_gpu_reveal_slots.py``.
"""

import ctypes
import re
from pathlib import Path

import pytest

from neuralsteganography_amd import _lib, cover, stego
from neuralsteganography_amd.exceptions import ConfigurationError
from neuralsteganography_amd.lm.mock import MockLM

HEADER = Path(__file__).resolve().parents[1] / "include" / "nsg_coder.h"
C_ARG = {"ns_ctx*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p,
         "const ns_stream_quality*": ctypes.c_void_p, "ns_stream_state*": ctypes.c_void_p,
         "uint8_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p,
         "ns_step_trace*": ctypes.c_void_p, "const int32_t*": None,  # a device table (void*) or the host ban list
         "int64_t": ctypes.c_int64, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}


def test_version_and_export():
    assert _lib.version().startswith("nsgcoder 0.31.6")
    assert "ns_decode_step_streams" in _lib.EXPORTS and hasattr(_lib.lib(), "ns_decode_step_streams")


def test_binding_matches_the_header():
    text = HEADER.read_text()
    decl = re.search(r"int ns_decode_step_streams\((.*?)\);", text, re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    names = [a.rsplit(" ", 1)[1] for a in args]
    types = [a.rsplit(" ", 1)[0] for a in args]
    assert names == ["ctx", "d_logits", "ld", "B", "d_quality", "k_max", "d_tokens", "tok_stride", "d_length",
                     "d_state", "d_out_bits", "out_stride", "d_counts", "counts_stride", "d_out_token", "banned",
                     "nbanned", "d_trace", "step_flags", "hip_stream"]
    fn = _lib.lib().ns_decode_step_streams
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args)
    for name, ctype, bound in zip(names, types, fn.argtypes):
        want = C_ARG[ctype]
        if want is None:
            want = ctypes.POINTER(ctypes.c_int32) if name == "banned" else ctypes.c_void_p
        assert bound is want or (want is ctypes.c_void_p and bound is ctypes.c_void_p), (name, ctype, bound)


@pytest.mark.parametrize("kw", [dict(), dict(k_max=0), dict(tok_stride=0), dict(counts_stride=0), dict(quality=8)])
def test_a_null_context_is_refused_before_anything_is_touched(kw):
    """No context exists without a GPU; with a null one the entry returns NS_ERR_CONFIG whatever else it is given
    (pointers that would fault if they were followed)."""
    a = dict(quality=64, k_max=300, tok_stride=8, counts_stride=8)
    a.update(kw)
    ban = (ctypes.c_int32 * 2)(50256, 628)
    rc = _lib.lib().ns_decode_step_streams(None, 64, 50304, 4, a["quality"], a["k_max"], 64, a["tok_stride"], 64, 64,
                                           64, 128, 64, a["counts_stride"], 64, ban, 2, None, 0, None)
    assert rc == _lib.NS_ERR_CONFIG
    assert _lib.lib().ns_last_error(None)


# ------------------------------------------------------------------------------------------------------ front end
SECRETS = [b"alpha", "beta beta", b"gamma gamma gamma", b"d", bytes(range(32, 127)) * 2]
SEEDS = ["one two three. ", "x y ", "one two three. ", "the quick brown fox jumps. ", "a longer seed of seven words. "]
KW = dict(ecc="none", chunk_bytes=40)
BASE = {"temp": 0.9, "precision": 26, "topk": 300}
QS = [BASE, dict(BASE, top_k=80, temp=0.8), BASE, dict(BASE, top_k=70, temp=0.7), dict(BASE, top_k=80, temp=0.8)]
WANT = [s.encode() if isinstance(s, str) else s for s in SECRETS]


@pytest.fixture(autouse=True)
def fixed_msg_id(monkeypatch):
    monkeypatch.setattr(stego, "make_msg_id", lambda: "00000000-0000-4000-8000-000000000001")


class _RecordingLM(MockLM):
    """MockLM that records the (context, quality) of every list it decodes."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def decode_arithmetic(self, tokens, context, *, quality):
        self.seen.append((tuple(tokens), tuple(context), stego.normalise_quality(quality)))
        return MockLM.decode_arithmetic(self, tokens, context, quality=quality)


def _texts(lm):
    return cover.cover_generate_batch(SECRETS, seed_texts=SEEDS, lm=lm, quality_gate=False, **KW)


def _top_k(q):
    return stego._quality_args(q).get("top_k")


def test_texts_to_spans_with_qualities_equals_one_call_per_quality():
    lm = _RecordingLM()
    texts = _texts(lm)
    got = cover.texts_to_spans(texts, seed_texts=SEEDS, lm=lm, qualities=QS)
    seen = list(lm.seen)
    want = [None] * len(texts)
    for q in (QS[0], QS[1], QS[3]):
        members = [i for i, x in enumerate(QS) if x == q]
        res = cover.texts_to_spans([texts[i] for i in members], seed_texts=[SEEDS[i] for i in members], lm=lm,
                                   quality=q)
        for i, sp in zip(members, res):
            want[i] = sp
    assert got == want and [len(s) for s in got] == [1, 1, 1, 1, 5]
    # every list was decoded after its own seed with its own text's quality
    by_ctx = {tuple(lm.encode_seed(s)): {_top_k(q) for s2, q in zip(SEEDS, QS) if s2 == s} for s in SEEDS}
    assert seen and all(_top_k(q) in by_ctx[c] for _, c, q in seen)
    assert {_top_k(q) for _, _, q in seen} == {300, 80, 70}
    # slots alone: the mock has no slot path, the call is the one it was
    assert cover.texts_to_spans(texts, seed_texts=SEEDS, lm=lm, quality=BASE, slots=2) == \
        cover.texts_to_spans(texts, seed_texts=SEEDS, lm=lm, quality=BASE)


def test_cover_reveal_batch_with_attempts_equals_one_call_per_quality():
    lm = _RecordingLM()
    texts = _texts(lm)
    attempts = [cover.Attempt(seed, {k: v for k, v in q.items() if BASE.get(k) != v}, "alt-1" if q != BASE else "base")
                for seed, q in zip(SEEDS, QS)]
    lm.seen.clear()
    assert cover.cover_reveal_batch(texts, attempts=attempts, quality=BASE, lm=lm, ecc="none") == WANT
    # the packets of a cover are decoded with the cover's quality too (stego_decode_batch(qualities=...))
    per_text = {tuple(lm.encode_seed(s)): set() for s in SEEDS}
    for _, c, q in lm.seen:
        per_text[c].add((_top_k(q), q.get("temp")))
    assert per_text[tuple(lm.encode_seed(SEEDS[3]))] == {(70, 0.7)}
    assert per_text[tuple(lm.encode_seed(SEEDS[0]))] == {(300, 0.9)}
    assert cover.cover_reveal_batch(texts, seed_texts=SEEDS, qualities=QS, lm=lm, ecc="none") == WANT
    for q in (QS[0], QS[1], QS[3]):
        members = [i for i, x in enumerate(QS) if x == q]
        assert cover.cover_reveal_batch([texts[i] for i in members], seed_texts=[SEEDS[i] for i in members],
                                        quality=q, lm=lm, ecc="none") == [WANT[i] for i in members]
    assert cover.cover_reveal(texts[4], seed_text=SEEDS[4], quality=QS[4], lm=lm, ecc="none", slots=1) == WANT[4]


def test_attempts_exclude_seeds_and_qualities():
    lm = MockLM()
    texts = _texts(lm)
    attempts = [cover.Attempt(seed, {}, "base") for seed in SEEDS]
    for extra in (dict(seed_texts=SEEDS), dict(seed_text=SEEDS[0]), dict(qualities=QS)):
        with pytest.raises(ConfigurationError, match="attempts"):
            cover.cover_reveal_batch(texts, attempts=attempts, lm=lm, ecc="none", **extra)


def test_wrong_lengths_are_refused():
    lm = MockLM()
    texts = _texts(lm)
    with pytest.raises(ConfigurationError, match="4 attempts for 5 covers"):
        cover.cover_reveal_batch(texts, attempts=[cover.Attempt(s, {}, "base") for s in SEEDS[:4]], lm=lm, ecc="none")
    with pytest.raises(ConfigurationError, match="4 qualities for 5 texts"):
        cover.cover_reveal_batch(texts, seed_texts=SEEDS, qualities=QS[:4], lm=lm, ecc="none")
    with pytest.raises(ConfigurationError, match="6 qualities for 5 texts"):
        cover.texts_to_spans(texts, seed_texts=SEEDS, qualities=QS + [BASE], lm=lm)
    with pytest.raises(ConfigurationError, match="exactly one of quality"):
        cover.texts_to_spans(texts, seed_texts=SEEDS, quality=BASE, qualities=QS, lm=lm)
    with pytest.raises(ConfigurationError, match="slots"):
        cover.texts_to_spans(texts, seed_texts=SEEDS, quality=BASE, slots=0, lm=lm)
