"""Case table of the rank coder's vocabulary suite, shared by ``tests/test_rank_vocab_host.py`` (CPU: the geometry the
ids claim, the oracle run of every case, a numpy restatement of the reference's formulas) and
``tests/test_gpu_rank_vocab.py`` (``ns_rank_encode_step`` / ``ns_rank_decode_step`` / ``ns_token_probs`` against those
oracle runs).  Nothing here touches the GPU or loads the HIP library.

The rank step of a logit row (``nsg_wide.hip``) is ``wide_stats_kernel`` (one wave per stream reads the row as tiles
of ``64 * W`` ids, W = 4 fp32 / 8 fp16, the last tile masked) -> ``wide_collect_kernel`` (one 256-thread block and one
counter atomic per 4096-id chunk, 49-bit keys carrying 17-bit ids) -> the segmented device sort ->
``wide_rank_kernel`` (1024 threads per stream; the row sum and the top_p prefix are staged through LDS in rounds of
8192 ranks).  A provider's float64 row goes through ``wide_rank64_kernel``, whose ``block_np_sum`` restates numpy's
pairwise sum (leaves ``< 8`` / ``<= 128``, splits at n/2 rounded down to a multiple of 8, 8192-element chunks).

The coder itself uses the support size n only through c = floor(log2 n); every expected step here carries n, which
the kernel reports in its step trace.
"""

from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from neuralsteganography_amd import synthetic
from oracle import oracle
from tests.golden.providers import near_tie_values

B = 5                           # streams per logit case
PAYLOAD_BYTES = (6, 5, 7, 3, 6)  # the streams finish at different steps
DEFAULT_SEED = 61
MAX_STEPS = 64                  # 56 payload bits at c >= 1
MAX_VOCAB = 0x1FFFF             # 17-bit ids
# constants of nsg_wide.hip, restated (tests/test_rank_vocab_host.py derives the claimed geometry from them)
WAVE, WIDE_THREADS, COLLECT_CHUNK, WIDE_ROUND = 64, 1024, 4096, 8192
TILE = {"f32": WAVE * 4, "f16": WAVE * 8}
NP_CHUNK, NP_LEAF, NP_UNROLL = 8192, 128, 8

# (V, the edge it claims)
VOCABS: List[Tuple[int, str]] = [
    (2, "smallest"),
    (3, "three-ids-c1"),
    (255, "f32-tile-less-1"),
    (256, "f32-tile"),
    (257, "f32-tile-plus-1"),
    (511, "f16-tile-less-1"),
    (512, "f16-tile"),
    (513, "f16-tile-plus-1"),
    (1023, "threads-less-1"),
    (1025, "threads-plus-1"),
    (4095, "chunk-less-1"),
    (4096, "chunk-no-pad"),
    (4097, "chunk-plus-1"),
    (8191, "round-less-1"),
    (8192, "round"),
    (8193, "round-plus-1"),
    (16385, "two-rounds-plus-1"),
    (65536, "ids-reach-16-bits"),
    (65537, "ids-cross-16-bits"),
    (100003, "prime"),
    (131071, "limit"),
]
DTYPES = ("f32", "f16")
CAP_MAX_VOCAB = 8193  # the oracle's 60-step cap bisection is 60 log/exp passes over the row: kept to the small rows


def policies(V: int):
    """(name, quality, temp, scale) for vocabulary V.  The filtering policies need rows with room to cut: at V = 2 and
    3 a cut leaves n < 2 at some step (no capacity), so those rows take the policies that keep every id."""
    below = max(2, (2 * V) // 3)
    half = max(2, V // 2)
    out = [
        ("none", {}, 1.0, 3.0),
        ("topk-equal", {"top_k": V}, 0.7, 3.0),
        ("topk-above", {"top_k": V + 5}, 1.5, 3.0),
        ("ptemp0.7", {"prob_temp": 0.7}, 1.0, 3.0),
        ("ptemp1.0-topk", {"prob_temp": 1.0, "top_k": below}, 1.0, 3.0),
    ]
    if V >= 255:
        out += [
            ("topk-below", {"top_k": below}, 1.0, 6.0),
            ("topp", {"top_p": 0.9}, 1.5, 3.0),
            ("minprob", {"min_prob": 0.5 / V}, 0.7, 3.0),
            ("combined", {"top_k": half, "top_p": 0.95, "min_prob": 0.05 / V}, 1.5, 3.0),
            ("ptemp1.3-topp", {"prob_temp": 1.3, "top_p": 0.9}, 1.5, 3.0),
        ]
    if 255 <= V <= CAP_MAX_VOCAB:
        out += [
            ("cap3", {"cap_per_token_bits": 3}, 1.0, 3.0),
            ("cap4-topk", {"cap_per_token_bits": 4, "top_k": half}, 1.0, 6.0),
        ]
    return out


# case id -> seed, where the default seed's rows do not qualify (tests/test_rank_vocab_host.py says what qualifies):
# each entry states why it left the default
SEEDS: Dict[str, int] = {}


class Case(NamedTuple):
    vocab: int
    dtype: str
    kind: str                 # "synthetic" | "constant" | "fixed" | "neginf" | "dominant"
    policy: str
    qitems: Tuple[Tuple[str, float], ...]
    temp: float
    scale: float
    seed: int
    err: Tuple[int, ...]      # the streams that end in a range error (no capacity)
    id: str

    @property
    def quality(self) -> dict:
        if self.kind == "fixed":
            return {"min_prob": exact_p_at_rank(self, FIXED_RANK)}
        return dict(self.qitems)

    @property
    def npdt(self):
        return np.float16 if self.dtype == "f16" else np.float32

    @property
    def exact_policy(self) -> bool:
        """Neither cap nor prob_temp: the kernel's arithmetic is the canonical one throughout."""
        return not ({"cap_per_token_bits", "prob_temp"} & set(self.quality))


def _case(vocab, dtype, kind, policy, quality, temp, scale, err, cid) -> Case:
    return Case(vocab, dtype, kind, policy, tuple(sorted(quality.items())), float(temp), float(scale),
                SEEDS.get(cid, DEFAULT_SEED), tuple(err), cid)


DOMINANT_STREAM = 2
# rank 712 and not a rounder one: the threshold equals the oracle's p of that rank to the last bit, and numpy's own
# quotient for the same rank lies an ulp below it for most ranks of the fp16 row (690 .. 711 among them), where numpy
# would keep one id fewer; 712 is the first rank from 690 up at which numpy and the oracle agree for both dtypes
FIXED_VOCAB, FIXED_RANK = 1025, 712
NEGINF_VOCABS = (257, 4097, 8193, 65537)
DOMINANT_VOCABS = (257, 8193, 131071)


def _cases() -> List[Case]:
    out = []
    for vocab, why in VOCABS:
        for dtype in DTYPES:
            for name, q, temp, scale in policies(vocab):
                out.append(_case(vocab, dtype, "synthetic", name, q, temp, scale, (),
                                 f"v{vocab}-{why}-{dtype}-{name}"))
    for dtype in DTYPES:
        # constant rows: p = 1/V exactly and every partial sum exact (V a power of two), so the cut ranks are known
        out += [
            _case(4096, dtype, "constant", "topp-half", {"top_p": 0.5}, 1.0, 0.0, (), f"const4096-{dtype}-topp0.5-n2048"),
            _case(16384, dtype, "constant", "topp-round-end", {"top_p": 0.5}, 1.0, 0.0, (),
                  f"const16384-{dtype}-topp0.5-cut8191-last-of-round"),
            _case(16384, dtype, "constant", "topp-round-start", {"top_p": 0.5 + 1.0 / 16384}, 1.0, 0.0, (),
                  f"const16384-{dtype}-topp0.5+1ulp-cut8192-first-of-round"),
            _case(16384, dtype, "constant", "minprob-all", {"min_prob": 1.0 / 16384}, 1.0, 0.0, (),
                  f"const16384-{dtype}-minprob-1/V-all-kept"),
            _case(16384, dtype, "constant", "minprob-none", {"min_prob": float(np.nextafter(1.0 / 16384, 1.0))}, 1.0, 0.0,
                  tuple(range(B)), f"const16384-{dtype}-minprob-next-above-1/V-none-kept"),
        ]
        # one row for every stream and step, min_prob = the probability of rank FIXED_RANK to the last bit (found by
        # bisection on the oracle's support, exact_p_at_rank): ``>=`` keeps FIXED_RANK + 1 ids, ``>`` one fewer, and
        # both give the same c
        out.append(_case(FIXED_VOCAB, dtype, "fixed", "minprob-exact", {}, 1.0, 3.0, (),
                         f"fixed{FIXED_VOCAB}-{dtype}-minprob-equals-p-of-rank-{FIXED_RANK}"))
        for vocab in NEGINF_VOCABS:
            for name, q in (("none", {}), ("topp", {"top_p": 0.9}), ("minprob0", {"min_prob": 0.0})):
                out.append(_case(vocab, dtype, "neginf", name, q, 1.5, 3.0, (), f"neginf{vocab}-{dtype}-{name}"))
        for vocab in DOMINANT_VOCABS:
            out.append(_case(vocab, dtype, "dominant", "topp", {"top_p": 0.9}, 1.5, 3.0, (DOMINANT_STREAM,),
                             f"dominant{vocab}-{dtype}-topp"))
    return out


CASES: List[Case] = _cases()


def payload(s: int) -> bytes:
    return synthetic.payload_bytes(s, PAYLOAD_BYTES[s % len(PAYLOAD_BYTES)])


def neginf_block(vocab: int) -> Tuple[int, int]:
    return vocab // 3, vocab // 3 + max(1, vocab // 4)


def case_row(case: Case, s: int, t: int) -> np.ndarray:
    """Row (s, t) as the kernel reads it (the case's dtype); the oracle sees it widened to float32."""
    V = case.vocab
    if case.kind == "constant":
        return np.full(V, 0.5, case.npdt)
    if case.kind == "fixed":
        return synthetic.logits_row(case.seed, 0, 0, V, case.scale, case.npdt)
    x = synthetic.logits_row(case.seed, s, t, V, case.scale, case.npdt)
    if case.kind == "neginf":
        a, b = neginf_block(V)
        x[a:b] = -np.inf
    elif case.kind == "dominant" and s == DOMINANT_STREAM:
        x[(7 * t + 3) % V] = case.npdt(float(x.max()) + 40.0)
    return x


def oracle_support(row: np.ndarray, temp: float, quality) -> int:
    """The oracle's support size n of one row (steps R1-R3), whatever its capacity."""
    one = np.zeros(1, np.uint8)
    return oracle.rank_step_n(np.asarray(row, dtype=np.float32), oracle.new_state(1), temp=temp, quality=quality,
                              payload=one, nbits=8)[4]


@functools.lru_cache(maxsize=None)
def exact_p_at_rank(case: Case, rank: int) -> float:
    """The largest double m with n(min_prob = m) > rank on the case's row, i.e. the oracle's p of that rank exactly:
    n(m) does not grow with m, and positive doubles are ordered as their bit patterns."""
    row = case_row(case, 0, 0)
    n_of = lambda m: oracle_support(row, case.temp, {"min_prob": float(m)})  # noqa: E731
    lo, hi = np.array([0.0]).view(np.uint64)[0], np.array([1.0]).view(np.uint64)[0]
    assert n_of(0.0) > rank >= n_of(1.0)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if n_of(np.array([mid], np.uint64).view(np.float64)[0]) > rank:
            lo = mid
        else:
            hi = mid
    return float(np.array([lo], np.uint64).view(np.float64)[0])


class Geometry(NamedTuple):
    tiles: int        # wide_stats_kernel: tiles of 64 * W ids
    last_tile: int    # ids in the last tile
    chunks: int       # wide_collect_kernel: blocks (and counter atomics) per row
    last_chunk: int   # ids in the last chunk
    rounds: int       # wide_rank_kernel: LDS staging rounds of the row sum and of the top_p prefix
    last_round: int   # ranks in the last round
    passes: int       # strided passes of the 1024 threads over the ranks


def geometry(vocab: int, dtype: str) -> Geometry:
    def split(n, unit):
        k = (n + unit - 1) // unit
        return k, n - (k - 1) * unit

    return Geometry(*split(vocab, TILE[dtype]), *split(vocab, COLLECT_CHUNK), *split(vocab, WIDE_ROUND),
                    split(vocab, WIDE_THREADS)[0])


def payload_index(pl: bytes, bit_pos: int, c: int) -> Tuple[int, int]:
    """(rank index, bits taken): the next c payload bits, MSB-first per byte, zero padded past the end."""
    idx = take = 0
    for t in range(c):
        bp = bit_pos + t
        bit = 0
        if bp < 8 * len(pl):
            bit = (pl[bp >> 3] >> (7 - (bp & 7))) & 1
            take += 1
        idx = (idx << 1) | bit
    return idx, take


class Stream(NamedTuple):
    payload: bytes
    steps: Tuple[Tuple[int, int, int, int, int], ...]  # (n, c, sel, take, token) per step
    status: str                                        # "done" | "range"
    err_n: int                                         # the support at the step that had no capacity (else -1)
    decoded: bytes                                     # the oracle's decode of its own tokens

    @property
    def tokens(self) -> List[int]:
        return [st[4] for st in self.steps]

    @property
    def consumed(self) -> List[int]:
        return [st[3] for st in self.steps]


def _oracle_stream(step_fn, pl: bytes) -> Stream:
    """One stream through the oracle alone.  ``step_fn(t, state, **kw)`` runs or_rank_step[64]_n on step t's row."""
    buf = np.frombuffer(pl, dtype=np.uint8).copy()
    nbits = 8 * len(pl)
    st = oracle.new_state(1)
    steps, status, err_n = [], "done", -1
    while st.bit_pos < nbits:
        t = len(steps)
        if t >= MAX_STEPS:
            raise RuntimeError(f"the oracle did not finish within {MAX_STEPS} steps")
        pos = int(st.bit_pos)
        rc, tok, take, c, n = step_fn(t, st, payload=buf, nbits=nbits)
        if rc == oracle.OR_ERR_RANGE:
            status, err_n = "range", n
            break
        if rc != oracle.OR_OK:
            raise RuntimeError(f"oracle rank step {t}: rc={rc}")
        sel, take2 = payload_index(pl, pos, c)
        assert take2 == take
        steps.append((n, c, sel, take, tok))
    dst = oracle.new_state(1)
    out = np.zeros(len(pl) + 8, dtype=np.uint8)
    for t, (n, c, sel, take, tok) in enumerate(steps):
        rc, _, keep, c2, n2 = step_fn(t, dst, token=tok, keep=take, out_bits=out)
        if rc != oracle.OR_OK or (keep, c2, n2) != (take, c, n):
            raise RuntimeError(f"oracle rank decode step {t}: rc={rc}")
    return Stream(pl, tuple(steps), status, err_n, out.tobytes()[: int(dst.bit_pos) // 8])


@functools.lru_cache(maxsize=None)
def expected(case: Case) -> Tuple[Stream, ...]:
    """The oracle's run of every stream of ``case`` (computed once per process; the GPU tests' expected values).
    The oracle sees ``row[:V]`` only -- no pad."""
    rq = oracle.rank_quality(case.quality)

    def run(s):
        def step(t, st, **kw):
            return oracle.rank_step_n(case_row(case, s, t).astype(np.float32), st, temp=case.temp, quality=rq, **kw)

        return _oracle_stream(step, payload(s))

    return tuple(run(s) for s in range(B))


# ----------------------------------------------------------------------------------------------- provider rows
PROVIDER_B = 3
PROVIDER_SEED = 67
# entry counts of stream 0 (streams 1 and 2 take the next two of the list: different counts in one batch)
COUNTS = [1, 2, 7, 8, 9, 127, 128, 129, 130, 135, 136, 255, 257, 4128, 8191, 8192, 8193, 8200, 16385, 131071]
PROVIDER_POLICIES = [
    ("none", {}),
    ("topp", {"top_p": 0.6}),
    ("minprob-topk", {"min_prob": 1e-6, "top_k": 5000}),
    ("crypto", {"prob_temp": 0.8}),
]
DICT_ID_SPACE = 1 << 20  # dict ids are drawn from here: most exceed 2^17


class ProviderCase(NamedTuple):
    counts: Tuple[int, ...]
    form: str                 # "ndarray" | "dict"
    policy: str
    qitems: Tuple[Tuple[str, float], ...]
    id: str

    @property
    def quality(self) -> dict:
        return dict(self.qitems)


def _provider_cases() -> List[ProviderCase]:
    out = []
    for i, n in enumerate(COUNTS):
        counts = tuple(COUNTS[(i + k) % len(COUNTS)] for k in range(PROVIDER_B))
        for form in ("ndarray", "dict"):
            for name, q in PROVIDER_POLICIES:
                out.append(ProviderCase(counts, form, name, tuple(sorted(q.items())), f"n{n}-{form}-{name}"))
    return out


PROVIDER_CASES: List[ProviderCase] = _provider_cases()


def provider_dist(case: ProviderCase, s: int, t: int):
    """Stream s's ProbDist at step t: near-tied float64 values (``tests/golden/providers.py``), so the order of
    summation changes the last bits of every total; a dict's ids are spread over 2^20."""
    n = case.counts[s]
    rng = np.random.default_rng([PROVIDER_SEED, n, s, t])
    vals = near_tie_values(rng, n, 1.05, 0.79)
    if case.form == "ndarray":
        return vals
    ids = rng.choice(DICT_ID_SPACE, size=n, replace=False)
    return {int(i): float(p) for i, p in zip(ids, vals)}


def provider_payload(s: int) -> bytes:
    return synthetic.payload_bytes(10 + s, (6, 4, 5)[s % 3])


@functools.lru_cache(maxsize=None)
def provider_expected(case: ProviderCase) -> Tuple[Stream, ...]:
    rq = oracle.rank_quality(case.quality)

    def run(s):
        def step(t, st, **kw):
            return oracle.rank_step64_n(provider_dist(case, s, t), st, quality=rq, **kw)

        return _oracle_stream(step, provider_payload(s))

    return tuple(run(s) for s in range(PROVIDER_B))


def np_sum_leaves(n: int) -> List[int]:
    """Leaf lengths of numpy's float64 sum over n elements, in order (the structure ``block_np_sum`` restates)."""
    out = []

    def rec(m):
        if m <= NP_LEAF:
            out.append(m)
        else:
            h = m // 2
            h -= h % NP_UNROLL
            rec(h)
            rec(m - h)

    for c0 in range(0, n, NP_CHUNK):
        rec(min(NP_CHUNK, n - c0))
    return out
