"""Case table of the decode step's divergence suite, shared by ``tests/test_decode_diverge_host.py`` (CPU: every
bad-token class holds in the oracle run, and the oracle's kept ids equal a numpy re-derivation) and
``tests/test_gpu_decode_diverge.py`` (``ns_decode_step`` against those oracle runs).  Nothing here touches the GPU or
loads the HIP library at import.

A case is one coder configuration with B = 6 streams of 10-14 tokens.  The oracle encodes a payload per stream on
``synthetic.logits_row`` rows (one row of one stream masked to a few finite logits); the first T tokens are the
stream's clean list.  The oracle then decodes the clean list step by step, which gives the state before every step,
the trace, the bytes written and the ids of ranks ``0 .. k'-1`` (``oracle.decode_step_kept``).  Every stream receives
one BAD token at one step, of a class chosen from that run:

    a      the id at rank k' on a step where k' < k (the overfill trim)
    b      the id at rank k (the first one cut by 1/R or by topk)
    c      the lowest-ranked valid id of the row
    d628   banned id 628            dV1   banned id V - 1
    e-1    -1      eV   V           eld   ld - 1, a poisoned pad column that must never be read
    f      an id whose logit is -inf (on the stream's masked row)
    g      the stream's last token (``is_last`` set) diverging: the id at rank k of that step

Six streams cannot carry ten bad tokens, so every configuration is two cases, ``v0`` and ``v1``, that assign the
classes differently (``ASSIGN``); the two together hold every class.  The controls -- the ids at rank k' - 1 and at
rank 0 of the same step, which must NOT diverge -- are recorded for every stream.

The precisions are low (10-16 bits) on purpose: at the suite's usual 26 bits the 1/R cutoff keeps every id of a
257-id row and the rounded masses never overfill, so neither class a nor b nor c would exist.
"""

from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from neuralsteganography_amd import synthetic
from oracle import oracle
from tests import coder_vocab_cases as cv

B = 6
DEFAULT_SEED = 41
MASK_STEP = 4          # the step whose row is masked (the class-f stream only)
MASK_FINITE = 24       # finite logits left on the masked row
WIDE_LDS_KEYS = 6144   # keys one stream sorts in LDS on the wide path (NSG_FAST_NL); more take the sweep / device sort

# class of stream s, per variant
ASSIGN = {
    0: ("a", "b", "c", "d628", "e-1", "f"),
    1: ("dV1", "eV", "eld", "g", "a", "c"),
}
CLASSES = ("a", "b", "c", "d628", "dV1", "e-1", "eV", "eld", "f", "g")

# per-stream (topk, temp, precision) of the quality-table family: they differ in all three
QUALITIES = [(100, 0.7, 12), (300, 0.9, 14), (512, 1.0, 16), (60, 1.2, 11), (200, 0.8, 13), (768, 1.1, 15)]

# (family, V, dtype, precision, topk, temp, scale)
CONFIGS = [
    ("single", 257, "f32", 12, 300, 0.9, 3.0),
    ("single", 257, "f16", 12, 100, 0.9, 3.0),
    ("single", 1025, "f32", 14, 300, 0.9, 3.0),
    ("single", 1025, "f16", 12, 100, 0.9, 3.0),
    ("sample", 8193, "f32", 10, 100, 0.9, 3.0),
    ("sample", 8193, "f16", 10, 100, 0.9, 3.0),
    ("quality", 1025, "f32", 16, 768, 1.0, 3.0),   # precision / topk / temp of each stream: QUALITIES
    ("wide-lds", 1025, "f32", 16, 50000, 1.0, 3.0),
    ("wide-lds", 1025, "f16", 16, 50000, 1.0, 3.0),
    ("wide-sweep", 32000, "f32", 16, 50000, 1.0, 2.0),
]

# (family, V, dtype, variant) -> seed, for a case whose default-seed rows give no step with k' < k where the table
# needs one
SEEDS: Dict[Tuple[str, int, str, int], int] = {
    ("single", 1025, "f16", 0): 42,
    ("wide-lds", 1025, "f16", 0): 42,
}


class Case(NamedTuple):
    family: str
    vocab: int
    dtype: str
    precision: int
    topk: int
    temp: float
    scale: float
    variant: int
    seed: int
    id: str

    @property
    def npdt(self):
        return np.float16 if self.dtype == "f16" else np.float32

    @property
    def banned(self) -> List[int]:
        return [self.vocab - 1, 628]

    @property
    def ld(self) -> int:
        """Row stride: ``coder.row_stride``, and 64 more columns where that leaves no pad column."""
        rs = ((self.vocab + 63) // 64) * 64
        return rs if rs > self.vocab else rs + 64

    def quality(self, s: int) -> Tuple[int, float, int]:
        """(topk, temp, precision) of stream s."""
        return QUALITIES[s] if self.family == "quality" else (self.topk, self.temp, self.precision)


def _cases() -> List[Case]:
    out = []
    for family, vocab, dtype, precision, topk, temp, scale in CONFIGS:
        for variant in (0, 1):
            seed = SEEDS.get((family, vocab, dtype, variant), DEFAULT_SEED)
            out.append(Case(family, vocab, dtype, precision, topk, temp, scale, variant, seed,
                            f"{family}-v{vocab}-{dtype}-p{precision}-k{topk}-v{variant}"))
    return out


CASES: List[Case] = _cases()
SINGLE_PASS_FAMILIES = ("single", "sample", "quality")


def nsteps(s: int) -> int:
    return 10 + (2 * s) % 5  # 10, 12, 14, 11, 13, 10


def class_of(case: Case, s: int) -> str:
    return ASSIGN[case.variant][s]


def case_row(case: Case, s: int, t: int) -> np.ndarray:
    """Row (s, t) in the case's dtype.  The class-f stream's row MASK_STEP keeps MASK_FINITE finite logits, the rest
    are -inf (as ``test_masked_rows_match_oracle``)."""
    x = synthetic.logits_row(case.seed, s, t, case.vocab, case.scale, case.npdt)
    if class_of(case, s) == "f" and t == MASK_STEP:
        keep = np.random.default_rng([case.seed, s, t]).choice(case.vocab, size=MASK_FINITE, replace=False)
        out = np.full(case.vocab, -np.inf, case.npdt)
        out[keep] = x[keep]
        return out
    return x


def numpy_order(row: np.ndarray, banned) -> np.ndarray:
    """Every non-banned id of ``row`` sorted by (value descending, id ascending): plain numpy, no oracle."""
    x = np.asarray(row, dtype=np.float64) + 0.0  # -0 -> +0
    ids = np.array([j for j in range(x.size) if j not in set(banned)], dtype=np.int64)
    return ids[np.lexsort((ids, -x[ids]))]


class Step(NamedTuple):
    state: Tuple[int, int, int, int]   # (lo, hi, bit_pos, ntokens) BEFORE the step
    trace: Tuple[int, int, int, int, int]  # (k, kprime, sel, n, token) of the clean token
    kept: Tuple[int, ...]              # ids of ranks 0 .. k'-1
    out: bytes                         # the stream's output bytes AFTER the step (zeros beyond bit_pos)


class Stream(NamedTuple):
    tokens: List[int]                  # the clean list
    steps: List[Step]
    final: Tuple[int, int, int, int]   # state after the last step
    decoded: List[int]                 # every bit the oracle's decode of the clean list emits
    cls: str
    bad_step: int
    bad_token: int
    controls: Tuple[int, int]          # ids at rank k'-1 and rank 0 of the bad step: must decode


def _st(st) -> Tuple[int, int, int, int]:
    return (int(st.lo), int(st.hi), int(st.bit_pos), int(st.ntokens))


def set_state(values) -> "oracle.OrState":
    st = oracle.OrState()
    st.lo, st.hi, st.bit_pos, st.ntokens = values
    st.flags = 0
    return st


def out_bytes(case: Case) -> int:
    """Bytes of one stream's output row: every step may emit ``precision`` bits, plus the slack the sessions keep."""
    pmax = max(case.quality(s)[2] for s in range(B))
    return (14 * pmax + pmax + 7) // 8 + 8


def _oracle_stream(case: Case, s: int) -> Stream:
    topk, temp, precision = case.quality(s)
    kw = dict(banned=case.banned, temp=temp, precision=precision, topk=topk)
    T = nsteps(s)
    rows = [case_row(case, s, t).astype(np.float32) for t in range(T)]
    payload = np.frombuffer(synthetic.payload_bytes(s, 64), dtype=np.uint8).copy()
    st = oracle.new_state(precision)
    tokens = []
    for t in range(T):
        rc, tok, _ = oracle.encode_step(rows[t], st, payload, 8 * payload.size, **kw)
        if rc != oracle.OR_OK:
            raise RuntimeError(f"{case.id} stream {s}: oracle encode step {t} rc={rc}")
        tokens.append(tok)
    assert st.bit_pos < 8 * payload.size
    st = oracle.new_state(precision)
    out = np.zeros(out_bytes(case), dtype=np.uint8)
    steps = []
    for t in range(T):
        before = _st(st)
        rc, tr, kept = oracle.decode_step_kept(rows[t], st, tokens[t], t == T - 1, out, **kw)
        if rc != oracle.OR_OK:
            raise RuntimeError(f"{case.id} stream {s}: oracle decode step {t} rc={rc}")
        steps.append(Step(before, (tr.k, tr.kprime, tr.sel, tr.n, tr.token), tuple(kept), out.tobytes()))
    decoded = np.unpackbits(out, bitorder="little")[: st.bit_pos].astype(np.int64).tolist()
    ref, _ = oracle.decode_stream(lambda t: rows[t], tokens, **kw)
    assert ref == decoded

    cls = class_of(case, s)
    nvalid = cv.nvalid(case.vocab, case.banned)
    inner = [1 + (s + i) % (T - 2) for i in range(T - 2)]  # not the first or the last step; starts at step 1 + s

    def first(pred, what):
        for t in inner:
            if pred(steps[t].trace[0], steps[t].trace[1]):
                return t
        raise RuntimeError(f"{case.id} stream {s}: no step with {what}; give the case a seed in SEEDS")

    if cls == "a":
        wide_trim = [t for t in inner if steps[t].trace[1] + 2 <= steps[t].trace[0]]
        # a trim of two or more ranks where there is one: an export that ran to k instead of k' then writes past
        # the terminator's slot
        bt = wide_trim[0] if wide_trim else first(lambda k, kp: kp < k, "k' < k")
        bad =int(numpy_order(rows[bt], case.banned)[steps[bt].trace[1]])
    elif cls == "b":
        bt = first(lambda k, kp: k < nvalid, "k < valid ids")
        bad = int(numpy_order(rows[bt], case.banned)[steps[bt].trace[0]])
    elif cls == "c":
        bt = first(lambda k, kp: kp < nvalid, "k' < valid ids")
        bad = int(numpy_order(rows[bt], case.banned)[-1])
    elif cls == "g":
        bt = T - 1
        if not steps[bt].trace[0] < nvalid:
            raise RuntimeError(f"{case.id} stream {s}: the last step keeps every id; give the case a seed in SEEDS")
        bad = int(numpy_order(rows[bt], case.banned)[steps[bt].trace[0]])
    elif cls == "f":
        bt = MASK_STEP
        bad = next(j for j in range(case.vocab) if rows[bt][j] == -np.inf and j not in case.banned)
    else:
        bt = 2 + s  # a different step per stream
        bad = {"d628": 628, "dV1": case.vocab - 1, "e-1": -1, "eV": case.vocab, "eld": case.ld - 1}[cls]
    kp = steps[bt].trace[1]
    return Stream(tokens, steps, _st(st), decoded, cls, bt, bad, (steps[bt].kept[kp - 1], steps[bt].kept[0]))


@functools.lru_cache(maxsize=None)
def expected(case: Case) -> Tuple[Stream, ...]:
    """The oracle's run of every stream of ``case`` (once per process).  The oracle sees ``row[:V]`` only."""
    return tuple(_oracle_stream(case, s) for s in range(B))


def oracle_try(case: Case, s: int, t: int, token: int, is_last: Optional[bool] = None):
    """One oracle decode step of stream s at step t from the clean run's state, with ``token`` instead of the clean
    one: (rc, state after, trace tuple, kept ids, output bytes after)."""
    e = expected(case)[s]
    topk, temp, precision = case.quality(s)
    st = set_state(e.steps[t].state)
    prev = e.steps[t - 1].out if t else bytes(out_bytes(case))
    out = np.frombuffer(prev, dtype=np.uint8).copy()
    last = t == len(e.tokens) - 1 if is_last is None else is_last
    rc, tr, kept = oracle.decode_step_kept(case_row(case, s, t).astype(np.float32), st, token, last, out,
                                           banned=case.banned, temp=temp, precision=precision, topk=topk)
    return rc, _st(st), (tr.k, tr.kprime, tr.sel, tr.n, tr.token), kept, out.tobytes()
