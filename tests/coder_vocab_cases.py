"""Case table of the coder's vocabulary-size suite, shared by ``tests/test_coder_vocab_host.py`` (CPU: the geometry
classes the ids claim, and the oracle run of every case) and ``tests/test_gpu_coder_vocab.py`` (the HIP coder against
those oracle runs).  Nothing here touches the GPU.

The single-pass kernel (``nsg_coder.hip``) reads a row as tiles of ``TS = 64 * W`` ids (W = 4 fp32, 8 fp16).  At
``V >= 8192`` -- and only while the Poisson bound of ``spec_j_rule`` stays within 160 -- it first reads a stratified
sample of ``NSAMP = 4096 / TS`` whole tiles, tile ``s * space + space - 1`` with ``space = ntiles // NSAMP``; the
``ntiles % NSAMP`` remainder tiles fall to the last wave of the split form.  The wide one-pass kernel
(``nsg_wide.hip``) gives each of its 8 waves ``ceil(ntiles / 8)`` tiles and carries 17-bit ids (V <= 131071).
"""

from __future__ import annotations

import ctypes
import functools
from typing import List, NamedTuple, Tuple

import numpy as np

from neuralsteganography_amd import _lib, synthetic
from oracle import oracle

B = 3                 # streams per case: one per pad poison (NaN, +inf, largest finite)
DEFAULT_SEED = 41
MAX_STEPS = 200       # a stream that has not finished by then has stalled in the reference's interval
WIDE_WAVES = 8        # waves of the wide one-pass kernel
WIDE_MAX_VOCAB = 0x1FFFF
# ns_max_topk per dtype (CAND - TS), restated so that importing this module loads no native library (pytest imports
# it at collection, before torch); tests/test_coder_vocab_host.py checks it against the library
SINGLE_PASS_MAX_TOPK = {"f32": 768, "f16": 512}

# (V, what it exercises)
VOCABS: List[Tuple[int, str]] = [
    (65, "one-partial-tile"),
    (257, "two-tiles-k-clamps"),
    (515, "smallest-f16-wide"),
    (771, "smallest-f32-wide-empty-waves"),
    (1025, "mid-no-sample"),
    (4096, "mid-no-sample-no-pad"),
    (8191, "largest-without-sample"),
    (8192, "smallest-with-sample-space2-rem0-no-pad"),
    (8193, "one-id-last-tile-rem1"),
    (12288, "space3-rem0-no-pad"),
    (15871, "f16-rem7-partial-last-tile"),
    (16127, "f32-rem15"),
    (32000, "provider-vocab"),
    (65536, "ids-reach-16-bits"),
    (65537, "ids-cross-16-bits"),
    (100003, "prime"),
    (131071, "wide-limit"),
    (151936, "single-pass-only"),
]

# (dtype, precision, topk, temp, scale, purpose)
CONFIGS = [
    ("f32", 26, 300, 0.9, 3.0, "base"),
    ("f16", 26, 100, 0.9, 3.0, "base"),
    ("f32", 26, 100, 0.9, 3.0, "sample-on-at-8192"),
    ("f32", 30, 768, 1.0, 3.0, "max-topk"),
    ("f16", 20, 512, 1.5, 1.0, "max-topk"),
    ("f32", 16, 50000, 1.0, 3.0, "wide"),
    ("f16", 22, 2000, 0.9, 6.0, "wide"),
]

# (V, dtype, topk) -> seed, for a case whose default-seed rows stall the reference's interval
SEEDS = {}


class Case(NamedTuple):
    vocab: int
    dtype: str
    precision: int
    topk: int
    temp: float
    scale: float
    seed: int
    id: str

    @property
    def npdt(self):
        return np.float16 if self.dtype == "f16" else np.float32

    @property
    def banned(self) -> List[int]:
        return [self.vocab - 1, 628]  # CoderParams' default, the reference's two banned ids


def dtype_code(dtype: str) -> int:
    return _lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32


def nvalid(vocab: int, banned) -> int:
    return vocab - len({b for b in banned if 0 <= b < vocab})


def is_wide(vocab: int, dtype: str, topk: int, banned=None) -> bool:
    """The context's path: K = min(topk, valid ids) beyond the single-pass limit takes the wide path."""
    banned = [vocab - 1, 628] if banned is None else banned
    return min(topk, nvalid(vocab, banned)) > SINGLE_PASS_MAX_TOPK[dtype]


class Geometry(NamedTuple):
    ts: int       # ids per tile
    nsamp: int    # sample tiles of the single-pass kernel
    ntiles: int
    space: int    # sample tile spacing (single pass, sample on)
    rem: int      # tiles beyond NSAMP * space: the split form's last wave takes them
    last: int     # ids in the last tile


def geometry(vocab: int, dtype: str) -> Geometry:
    ts = 64 * (8 if dtype == "f16" else 4)
    nsamp = 4096 // ts
    ntiles = (vocab + ts - 1) // ts
    return Geometry(ts, nsamp, ntiles, ntiles // nsamp, ntiles % nsamp, vocab - (ntiles - 1) * ts)


def spec_j(vocab: int, topk: int, temp: float = 1.0, precision: int = 26, banned=None) -> int:
    """The library's own sample rule (``ns_stream_quality_fill``): 0 = the stratified sample is off."""
    banned = [vocab - 1, 628] if banned is None else banned
    row = _lib.NsStreamQuality()
    ban = (ctypes.c_int32 * max(1, len(banned)))(*banned)
    rc = _lib.lib().ns_stream_quality_fill(vocab, ban, len(banned), float(temp), int(topk), int(precision), int(topk),
                                           ctypes.byref(row))
    assert rc == _lib.NS_OK, _lib.lib().ns_last_error(None)
    return int(row.spec_j)


def sample_on(vocab: int, dtype: str, topk: int) -> bool:
    return not is_wide(vocab, dtype, topk) and spec_j(vocab, min(topk, SINGLE_PASS_MAX_TOPK[dtype])) > 0


def _cases() -> List[Case]:
    out = []
    for vocab, why in VOCABS:
        for dtype, precision, topk, temp, scale, purpose in CONFIGS:
            if vocab > WIDE_MAX_VOCAB and is_wide(vocab, dtype, topk):
                continue  # the wide path carries 17-bit ids: refused at context creation (tested on its own)
            seed = SEEDS.get((vocab, dtype, topk), DEFAULT_SEED)
            out.append(Case(vocab, dtype, precision, topk, temp, scale, seed,
                            f"v{vocab}-{why}-{dtype}-p{precision}-k{topk}-{purpose}"))
    return out


CASES: List[Case] = _cases()
UNSUPPORTED_WIDE = [(v, d, p, k) for v, _ in VOCABS for d, p, k, _, _, _ in CONFIGS
                    if v > WIDE_MAX_VOCAB and is_wide(v, d, k)]


def payload_bits(s: int) -> List[int]:
    return synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 8))[: 48 - 5 * s]


def case_row(case: Case, s: int, t: int) -> np.ndarray:
    """Row (s, t) as the kernel reads it (the case's dtype)."""
    return synthetic.logits_row(case.seed, s, t, case.vocab, case.scale, case.npdt)


class Expected(NamedTuple):
    bits: List[int]                   # the payload
    tokens: List[int]
    traces: List[Tuple[int, ...]]     # (k, kprime, sel, n, token) per step
    decoded: List[int]                # every bit the oracle's decode emits for `tokens`


def oracle_stream(row_fn, bits, *, banned, temp, precision, topk) -> Expected:
    """One stream through the oracle alone: encode (every step OR_OK, done within MAX_STEPS), then decode."""
    packed = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    st = oracle.new_state(precision)
    toks, traces, rows = [], [], []
    while st.bit_pos < len(bits):
        t = len(toks)
        if t >= MAX_STEPS:
            raise RuntimeError(f"the oracle's interval stalled: bit {st.bit_pos} of {len(bits)} after {t} steps")
        rows.append(np.asarray(row_fn(t), dtype=np.float32))
        rc, tok, tr = oracle.encode_step(rows[-1], st, packed, len(bits), banned=banned, temp=temp,
                                         precision=precision, topk=topk)
        if rc != oracle.OR_OK:
            raise RuntimeError(f"oracle encode step {t}: rc={rc}")
        toks.append(tok)
        traces.append((tr.k, tr.kprime, tr.sel, tr.n, tr.token))
    decoded, _ = oracle.decode_stream(lambda t: rows[t], toks, banned=banned, temp=temp, precision=precision,
                                      topk=topk)
    return Expected(list(bits), toks, traces, decoded)


@functools.lru_cache(maxsize=None)
def expected(case: Case) -> Tuple[Expected, ...]:
    """The oracle's run of every stream of ``case`` (computed once per process; the GPU tests' expected values).
    The oracle sees ``row[:V]`` only -- no pad."""
    return tuple(oracle_stream(lambda t, s=s: case_row(case, s, t), payload_bits(s), banned=case.banned,
                               temp=case.temp, precision=case.precision, topk=case.topk) for s in range(B))
