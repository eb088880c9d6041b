"""Cases of the per-stream sampler step (``ns_sample_step_streams``) shared by the host and the GPU tests: B = 8
streams on synthetic rows, every stream with its own temperature, top-k, length, seed and draw id, and the oracle's
tokens and statistics for each (``oracle.sample_stream``, computed once per case)."""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from neuralsteganography_amd import _lib, synthetic
from oracle import oracle

EVERY = -1  # top-k "every id"
TEMPS = (0.7, 0.9, 1.0, 1.3)
MAX_STEPS = 12


def limit(dtype: str) -> int:
    """The single-pass kernel's largest top-k (``ns_max_topk``: 768 for fp32 rows, 512 for fp16)."""
    return _lib.max_topk(_lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32)


@dataclass(frozen=True)
class Stream:
    temp: float
    topk: int  # EVERY: every id
    length: int
    seed: int
    gid: int


@dataclass(frozen=True)
class Case:
    name: str
    vocab: int
    dtype: str
    k_max: int  # EVERY: the vocabulary
    scale: float
    logit_seed: int
    streams: Tuple[Stream, ...]
    pad: int = 0  # elements added to the row stride

    @property
    def banned(self) -> List[int]:
        return [self.vocab - 1, 628]

    @property
    def npdt(self):
        return np.float16 if self.dtype == "f16" else np.float32

    def topk_of(self, s: int) -> int:
        """Stream s's top-k as the quality row takes it (every id: the vocabulary)."""
        k = self.streams[s].topk
        return k if k > 0 else self.vocab

    @property
    def k_max_row(self) -> int:
        return self.k_max if self.k_max > 0 else self.vocab


def _streams(topks, lengths, seed0) -> Tuple[Stream, ...]:
    return tuple(Stream(TEMPS[i % 4], k, n, seed0 + 7919 * i, 3 + 5 * i) for i, (k, n) in enumerate(zip(topks, lengths)))


NAMES = ("single_f32", "single_f16", "wide_f32", "small_vocab", "padded_stride")


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """The cases by name.  Built on first use, not at import: the single-pass limit comes from the library, which a
    test module must not load while it is being collected (before torch has brought up its own HIP runtime)."""
    f32, f16 = limit("f32"), limit("f16")
    lens = (12, 5, 12, 12, 1, 12, 5, 12)
    out = [
        Case("single_f32", 50257, "f32", f32, 3.0, 17, _streams((40, 2, 1, 100, 300, f32, 300, 40), lens, 0xC0FFEE)),
        Case("single_f16", 50257, "f16", f16, 3.0, 19, _streams((40, 2, 1, 100, 300, f16, 300, 40), lens, 0xBEEF01)),
        Case("wide_f32", 50257, "f32", EVERY, 3.0, 23,
             _streams((2000, f32 + 1, EVERY, 300, 2000, EVERY, f32 + 1, 300), lens, 0xABCDE1)),
        Case("small_vocab", 700, "f32", 690, 2.0, 29, _streams((690, 2, 690, 2, 690, 2, 690, 2), lens, 0x5EED05)),
        Case("padded_stride", 50257, "f32", 300, 3.0, 31,
             _streams((300, 2, 40, 100, 300, 1, 40, 100), lens, 0x0DDBA1), pad=64),
    ]
    assert tuple(c.name for c in out) == NAMES
    return {c.name: c for c in out}


def case(name: str) -> Case:
    return cases()[name]


def row_fn(case: Case, s: int):
    """Step t's logits of stream s, as the kernel reads them (fp16 rows rounded to fp16 first)."""
    return lambda t: synthetic.logits_row(case.logit_seed, s, t, case.vocab, case.scale, case.npdt).astype(np.float32)


def oracle_stream(case: Case, s: int, like: int = None):
    """``(tokens, stats accumulators)`` of stream s over its own length -- under its own temperature, top-k, seed
    and draw id, or (``like``) under those of stream ``like``."""
    q = case.streams[s if like is None else like]
    acc = np.zeros(4)
    toks, _ = oracle.sample_stream(row_fn(case, s), case.streams[s].length, banned=case.banned, temp=q.temp,
                                   topk=q.topk, seed=q.seed, gid=q.gid, stats=acc)
    return toks, acc


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """Per stream ``(tokens, accumulators)`` of case ``name`` (computed once, shared, never modified)."""
    c = case(name)
    return tuple(oracle_stream(c, s) for s in range(len(c.streams)))


def logits_batch(case: Case, order, t: int, ld: int) -> np.ndarray:
    """[len(order), ld] rows of step t for the streams ``order`` (row i = stream order[i])."""
    return synthetic.logits_batch(case.logit_seed, list(order), t, case.vocab, case.scale, case.npdt, ld)


# the provider-level inputs (tests/test_gpu_sample_batch_contexts.py): 7 messages, context lengths at the page and
# block edges, 5 distinct (temperature, top-k) pairs, 7 seeds
CONTEXT_LENGTHS = (1, 31, 32, 33, 64, 65, 100)
LENGTHS = (3, 40, 7, 1, 36, 12, 5)
PAIRS = ((1.0, 40), (0.7, 2), (1.3, 300), (0.9, 100), (1.0, 40), (0.7, 2), (1.1, 17))
SEEDS = (11, 2024, 0xC0FFEE, 5, 77, 123456789, (1 << 63) + 9)


def contexts(vocab: int = 512, seed: int = 4242) -> List[List[int]]:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, vocab - 1, size=n).tolist() for n in CONTEXT_LENGTHS]
