"""CPU side of the rank coder's vocabulary suite (``tests/rank_vocab_cases.py``): the geometry the case ids claim is
recomputed from the kernel's constants, every case runs through the oracle alone -- the values
``tests/test_gpu_rank_vocab.py`` expects of the HIP rank kernels -- and the oracle's support size n and tokens are
checked against a plain numpy float64 restatement of the reference's formulas (``lm/arithmetic.py:67-71`` softmax,
``codec/quality.py:57-105`` apply_quality, ``codec/arithmetic.py:122-168`` selection).
"""

import math

import numpy as np
import pytest

from oracle import oracle
from tests import rank_vocab_cases as rv
from tests.rank_vocab_cases import CASES, PROVIDER_CASES, geometry

EXACT = [c for c in CASES if c.exact_policy]
TOLERANT = [c for c in CASES if not c.exact_policy]  # cap / prob_temp: block sums and libm in the kernel


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------- the table
def test_table_holds_the_vocabularies_dtypes_and_policies():
    assert [v for v, _ in rv.VOCABS] == [2, 3, 255, 256, 257, 511, 512, 513, 1023, 1025, 4095, 4096, 4097, 8191, 8192,
                                         8193, 16385, 65536, 65537, 100003, 131071]
    assert len({c.id for c in CASES}) == len(CASES)
    for v, _ in rv.VOCABS:
        for dtype in rv.DTYPES:
            names = {c.policy for c in CASES if (c.vocab, c.dtype, c.kind) == (v, dtype, "synthetic")}
            assert {"none", "topk-equal", "topk-above", "ptemp0.7", "ptemp1.0-topk"} <= names
            if v >= 255:
                assert {"topk-below", "topp", "minprob", "combined", "ptemp1.3-topp"} <= names
            if 255 <= v <= rv.CAP_MAX_VOCAB:
                assert {"cap3", "cap4-topk"} <= names
    syn = [c for c in CASES if c.kind == "synthetic"]
    assert {c.temp for c in syn} >= {0.7, 1.0, 1.5} and {c.scale for c in syn} == {3.0, 6.0}
    assert {c.quality["prob_temp"] for c in syn if "prob_temp" in c.quality} == {0.7, 1.0, 1.3}
    for c in syn:
        k = c.quality.get("top_k")
        if c.policy in ("topk-below", "topk-equal", "topk-above"):
            assert (k < c.vocab, k == c.vocab, k > c.vocab) == tuple(c.policy == "topk-" + w
                                                                      for w in ("below", "equal", "above"))
    assert all(c.seed == rv.DEFAULT_SEED or c.id in rv.SEEDS for c in CASES)
    assert len(rv.PAYLOAD_BYTES) == rv.B == 5 and len(set(rv.PAYLOAD_BYTES)) > 2
    assert rv.COUNTS == [1, 2, 7, 8, 9, 127, 128, 129, 130, 135, 136, 255, 257, 4128, 8191, 8192, 8193, 8200, 16385,
                         131071]
    assert len(PROVIDER_CASES) == len(rv.COUNTS) * 2 * 4


@pytest.mark.parametrize("vocab,dtype,want", [
    (2, "f32", (1, 2, 1, 2, 1, 2, 1)), (255, "f32", (1, 255, 1, 255, 1, 255, 1)), (256, "f32", (1, 256, 1, 256, 1, 256, 1)),
    (257, "f32", (2, 1, 1, 257, 1, 257, 1)), (257, "f16", (1, 257, 1, 257, 1, 257, 1)),
    (511, "f16", (1, 511, 1, 511, 1, 511, 1)), (512, "f16", (1, 512, 1, 512, 1, 512, 1)),
    (513, "f16", (2, 1, 1, 513, 1, 513, 1)), (513, "f32", (3, 1, 1, 513, 1, 513, 1)),
    (1023, "f32", (4, 255, 1, 1023, 1, 1023, 1)), (1025, "f32", (5, 1, 1, 1025, 1, 1025, 2)),
    (4095, "f32", (16, 255, 1, 4095, 1, 4095, 4)), (4096, "f16", (8, 512, 1, 4096, 1, 4096, 4)),
    (4097, "f32", (17, 1, 2, 1, 1, 4097, 5)), (8191, "f16", (16, 511, 2, 4095, 1, 8191, 8)),
    (8192, "f32", (32, 256, 2, 4096, 1, 8192, 8)), (8193, "f32", (33, 1, 3, 1, 2, 1, 9)),
    (16385, "f16", (33, 1, 5, 1, 3, 1, 17)), (65536, "f32", (256, 256, 16, 4096, 8, 8192, 64)),
    (65537, "f16", (129, 1, 17, 1, 9, 1, 65)), (100003, "f32", (391, 163, 25, 1699, 13, 1699, 98)),
    (131071, "f32", (512, 255, 32, 4095, 16, 8191, 128)), (131071, "f16", (256, 511, 32, 4095, 16, 8191, 128))])
def test_geometry_of_the_named_vocabularies(vocab, dtype, want):
    g = geometry(vocab, dtype)
    assert tuple(g) == want
    assert (g.tiles - 1) * rv.TILE[dtype] + g.last_tile == vocab == (g.chunks - 1) * rv.COLLECT_CHUNK + g.last_chunk
    assert (g.rounds - 1) * rv.WIDE_ROUND + g.last_round == vocab


def test_vocabularies_claim_their_geometry_class():
    name = dict((v, w) for v, w in rv.VOCABS)
    g32 = {v: geometry(v, "f32") for v in name}
    g16 = {v: geometry(v, "f16") for v in name}
    # tiles: one id short of a tile, a full tile, one id in the next tile -- for each dtype's tile size
    assert [(g32[v].tiles, g32[v].last_tile) for v in (255, 256, 257)] == [(1, 255), (1, 256), (2, 1)]
    assert [(g16[v].tiles, g16[v].last_tile) for v in (511, 512, 513)] == [(1, 511), (1, 512), (2, 1)]
    assert [g32[v].passes for v in (1023, 1025)] == [1, 2]
    assert [(g32[v].chunks, g32[v].last_chunk) for v in (4095, 4096, 4097)] == [(1, 4095), (1, 4096), (2, 1)]
    assert 4096 % 64 == 0 and 16384 % 64 == 0, "row_stride == V: no pad columns at all"
    assert [(g32[v].rounds, g32[v].last_round) for v in (8191, 8192, 8193)] == [(1, 8191), (1, 8192), (2, 1)]
    assert (g32[16385].rounds, g32[16385].last_round) == (3, 1)
    assert 65536 - 1 < 1 << 16 <= 65537 - 1, "the last id of 65537 needs 17 bits"
    assert 131071 == rv.MAX_VOCAB == (1 << 17) - 1
    assert g32[100003].last_tile not in (1, rv.TILE["f32"]) and g32[100003].last_chunk == g32[100003].last_round
    assert {v for v in name if v <= 3} == {2, 3}  # c = 1 at every step
    # under {} the capacity is floor(log2 V) and a payload selects any rank of [0, 2^c): beyond the first staging
    # round from V = 16385 up, and into the last round at the limit
    assert [(1 << int(math.log2(v))) // rv.WIDE_ROUND for v in (8193, 16385, 65537, 131071)] == [1, 2, 8, 8]


def test_provider_counts_claim_their_leaf_structure():
    """numpy's pairwise sum: < 8 a plain loop, <= 128 one unrolled leaf (with a remainder when n % 8), above that a
    split at n/2 rounded down to a multiple of 8, 8192-element chunks added left to right."""
    lv = rv.np_sum_leaves
    assert [lv(n) for n in (1, 2, 7)] == [[1], [2], [7]]                      # plain loop
    assert [lv(n) for n in (8, 9, 127, 128)] == [[8], [9], [127], [128]]      # one leaf: no / some remainder
    assert lv(129) == [64, 65] and lv(130) == [64, 66]                        # the first split; 65 // 8 * 8 == 64
    assert lv(135) == [64, 71] and lv(136) == [64, 72]                        # n/2 = 67, 68 rounded down to 64
    assert lv(255) == [120] + lv(135)                                         # 127 -> 120; the right half splits again
    assert lv(257) == [128, 64, 65]
    assert lv(4128) == lv(2064) * 2 and sorted(set(lv(4128))) == [64, 72, 128]  # 258 = 128 + 130 -> 128 + 64 + 66 ...
    assert lv(8191) == lv(4088) + lv(4103) and sorted(set(lv(8191))) == [64, 71, 120, 128]
    assert len(lv(8192)) == 64 and set(lv(8192)) == {128}
    assert lv(8193) == lv(8192) + [1] and lv(8200) == lv(8192) + [8]          # a second chunk: plain loop / one leaf
    assert lv(16385) == lv(8192) * 2 + [1]
    assert len(lv(131071)) == 15 * 64 + len(lv(8191)) <= 2048                 # NP_MAX_LEAVES of the kernel
    for n in rv.COUNTS:
        assert sum(lv(n)) == n and max(lv(n)) <= rv.NP_LEAF
    x = np.random.default_rng(3).random(16385) * 1e-3
    for n in rv.COUNTS[:-1]:  # the structure is numpy's: the oracle's restatement equals numpy's own sum
        assert oracle.np_sum(x[:n]) == float(np.sum(x[:n]))


# ------------------------------------------------------------------------------------------ the oracle's runs
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_oracle_completes_every_stream(case):
    """The oracle alone: every stream finishes within the step bound, or is one the case names and ends in a range
    error; the oracle's decode of its own tokens gives the payload back."""
    exp = rv.expected(case)
    assert len(exp) == rv.B
    for s, e in enumerate(exp):
        assert e.payload == rv.payload(s)
        if s in case.err:
            assert e.status == "range" and e.err_n < 2 and e.decoded == e.payload[: len(e.decoded)]
            continue
        assert e.status == "done" and 1 <= len(e.steps) <= rv.MAX_STEPS
        assert sum(e.consumed) == 8 * len(e.payload) and e.decoded == e.payload
        for n, c, sel, take, tok in e.steps:
            assert 2 <= n <= case.vocab and 1 << c <= n < 2 << c and 0 <= sel < 1 << c and 0 <= tok < case.vocab
    done = [len(e.steps) for s, e in enumerate(exp) if s not in case.err]
    assert len(set(done)) > 1 or not done, "the streams finish at different steps"


def test_special_rows_are_what_their_ids_say():
    by = {c.id: rv.expected(c) for c in CASES if c.kind in ("constant", "fixed")}
    for dtype in rv.DTYPES:
        assert {st[0] for e in by[f"const4096-{dtype}-topp0.5-n2048"] for st in e.steps} == {2048}
        assert {st[0] for e in by[f"const16384-{dtype}-topp0.5-cut8191-last-of-round"] for st in e.steps} == {8192}
        assert {st[0] for e in by[f"const16384-{dtype}-topp0.5+1ulp-cut8192-first-of-round"] for st in e.steps} == {8193}
        assert {st[0] for e in by[f"const16384-{dtype}-minprob-1/V-all-kept"] for st in e.steps} == {16384}
        assert all(e.status == "range" and e.err_n == 0
                   for e in by[f"const16384-{dtype}-minprob-next-above-1/V-none-kept"])
        fixed = by[f"fixed{rv.FIXED_VOCAB}-{dtype}-minprob-equals-p-of-rank-{rv.FIXED_RANK}"]
        assert {st[0] for e in fixed for st in e.steps} == {rv.FIXED_RANK + 1}
        assert 1 << 9 < rv.FIXED_RANK < rv.FIXED_RANK + 1 < (1 << 10) - 1  # one id fewer: the same c, the same tokens
    for c in CASES:
        exp = rv.expected(c)
        if c.kind == "constant":  # equal logits: the order is id ascending, so the token is the selected rank
            assert all(st[2] == st[4] for e in exp for st in e.steps)
        if c.kind == "neginf":    # the -inf block is ranked last with zero mass: never in the support, never a token
            a, b = rv.neginf_block(c.vocab)
            assert all(st[0] <= c.vocab - (b - a) and not a <= st[4] < b for e in exp for st in e.steps)
            if c.policy in ("none", "minprob0"):
                assert all(st[0] == c.vocab - (b - a) for e in exp for st in e.steps)
        if c.kind == "dominant":
            assert exp[rv.DOMINANT_STREAM].status == "range" and exp[rv.DOMINANT_STREAM].err_n == 1
            assert not exp[rv.DOMINANT_STREAM].steps


def test_fp16_rows_beyond_65536_ids_tie_at_every_rank():
    """More ids than finite fp16 values: under {} the selectable ranks are full of equal logits, whose order must be
    id ascending."""
    for c in CASES:
        if c.dtype == "f16" and c.vocab >= 65537 and c.policy == "none" and c.kind == "synthetic":
            x = rv.case_row(c, 0, 0)
            assert np.unique(x).size < 65536 < x.size
            order = np.lexsort((np.arange(x.size), -x.astype(np.float64)))
            tied = x[order][1:] == x[order][:-1]
            assert tied.mean() > 0.5
            exp = rv.expected(c)
            assert all(st[0] == c.vocab for e in exp for st in e.steps)


# ------------------------------------------------------------------------------- numpy restatement (exact policies)
def numpy_support(x, temp, quality):
    """The reference's formulas in plain numpy float64: (ids in rank order, p in rank order, n)."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    z = x / temp
    p = np.exp(z - z.max())
    p /= p.sum()
    order = np.lexsort((np.arange(x.size), -x))
    ps = p[order]
    n = int(np.count_nonzero(ps > 0))
    assert np.all(ps[:n] > 0)
    if quality.get("top_k"):
        n = min(n, int(quality["top_k"]))
    if quality.get("top_p"):
        cut = int(np.searchsorted(np.cumsum(ps), quality["top_p"], side="left"))
        n = min(n, min(cut + 1, x.size))
    if quality.get("min_prob") is not None:
        keep = ps >= quality["min_prob"]
        n = min(n, x.size if keep.all() else int(np.argmin(keep)))
    return order, ps, n


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_oracle_support_and_tokens_match_numpy(case):
    """No step is excluded: a case whose numpy support differs from the oracle's at any step (a cumulative sum
    within an ulp of top_p, a probability within an ulp of min_prob) is not allowed in the table."""
    q = case.quality
    for s, e in enumerate(rv.expected(case)):
        pos = 0
        for t, (n, c, sel, take, tok) in enumerate(e.steps):
            order, _, n_np = numpy_support(rv.case_row(case, s, t), case.temp, q)
            assert n_np == n, f"stream {s} step {t}: numpy keeps {n_np}, the oracle {n}"
            c_np = int(math.floor(math.log2(n_np)))
            idx, took = rv.payload_index(e.payload, pos, c_np)
            assert (c_np, idx, took, int(order[idx])) == (c, sel, take, tok), f"stream {s} step {t}"
            pos += took
        if e.status == "range":
            _, _, n_np = numpy_support(rv.case_row(case, s, len(e.steps)), case.temp, q)
            assert n_np == e.err_n < 2


# ------------------------------------------------------------------ cap / prob_temp: robust to the order of summation
def fsum_support(x, temp, quality):
    """A second evaluation of the oracle's steps R1, R1c, R2, R3 with every sum taken by ``math.fsum`` (exactly
    rounded) and numpy's exp / log: the support size n."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    V = x.size
    order = np.lexsort((np.arange(V), -x))
    z = x[order] / temp
    e = np.exp(z - z[0])
    p = e / math.fsum(e.tolist())

    def prefix(a):
        zero = np.flatnonzero(a == 0.0)
        return int(zero[0]) if zero.size else V

    n = prefix(p)
    T = quality.get("prob_temp")
    if T and not math.isclose(T, 1.0):
        a = np.log(p + 1e-12) / T
        qv = np.exp(a - a[0])
        p = qv / math.fsum(qv.tolist())
        n = prefix(p)
    if quality.get("top_k"):
        n = min(n, int(quality["top_k"]))
    if quality.get("top_p"):
        cut = int(np.searchsorted(np.cumsum(p), quality["top_p"], side="left"))
        n = min(n, min(cut + 1, V))
    cap = quality.get("cap_per_token_bits")
    if cap and n > 0:
        def entropy(a):
            a = a[a > 0]
            return -math.fsum((a * np.log2(a)).tolist())

        f = np.zeros(V)
        f[:n] = p[:n] / math.fsum(p[:n].tolist())
        if entropy(f) > cap:
            low, high, target = 1e-6, 1.0, f
            lf = np.log(f + 1e-12)
            for _ in range(60):
                mid = (low + high) / 2.0
                cand = np.exp(lf / mid - lf[0] / mid)
                cand = cand / math.fsum(cand.tolist())
                if entropy(cand) > cap:
                    high = mid
                else:
                    low, target = mid, cand
            n = prefix(target)
    return n


@pytest.mark.parametrize("case", TOLERANT, ids=_ids(TOLERANT))
def test_cap_and_prob_temp_cases_do_not_depend_on_the_order_of_summation(case):
    """The kernel evaluates cap and prob_temp with block sums and the device's log / exp (tolerance-level).
    A case is kept only if the support of every step is the same under exactly rounded sums: then the comparison
    with the kernel is exact."""
    q = case.quality
    for s, e in enumerate(rv.expected(case)):
        for t, st in enumerate(e.steps):
            n = fsum_support(rv.case_row(case, s, t), case.temp, q)
            assert n == st[0], f"stream {s} step {t}: fsum keeps {n}, the oracle {st[0]}"


# ------------------------------------------------------------------------------------------ what only n protects
def _loose(n):
    """n is no power of two and n - 1, n + 1 have the same floor(log2): an off-by-one cut changes no token."""
    c = int(math.floor(math.log2(n)))
    return (1 << c) < n < (2 << c) - 1


@pytest.mark.parametrize("policy,binding", [
    ("topp", lambda case, x, n: n < case.vocab),
    ("minprob", lambda case, x, n: n < case.vocab),
    ("topk-below", lambda case, x, n: n == case.quality["top_k"]),
])
def test_each_filter_has_steps_that_only_the_support_size_protects(policy, binding):
    hits = 0
    for case in CASES:
        if case.policy != policy or case.kind != "synthetic":
            continue
        for s, e in enumerate(rv.expected(case)):
            hits += sum(1 for st in e.steps if _loose(st[0]) and binding(case, None, st[0]))
    assert hits >= 10, f"{policy}: {hits} steps whose tokens an off-by-one cut leaves unchanged"


# ---------------------------------------------------------------------------------------------- provider rows
@pytest.mark.parametrize("case", PROVIDER_CASES, ids=_ids(PROVIDER_CASES))
def test_oracle_completes_every_provider_stream(case):
    """Rows of one entry have no capacity (the reference's ArithmeticRangeError); every other stream finishes and
    decodes to its payload.  A dict's tokens are its ids (beyond 2^17), an ndarray's the positions."""
    exp = rv.provider_expected(case)
    for s, e in enumerate(exp):
        if case.counts[s] < 2:
            assert e.status == "range" and not e.steps
            continue
        assert e.status == "done" and e.decoded == e.payload == rv.provider_payload(s)
        assert all(2 <= st[0] <= case.counts[s] for st in e.steps)
        if case.form == "ndarray":
            assert all(0 <= st[4] < case.counts[s] for st in e.steps)
        else:
            d0 = rv.provider_dist(case, s, 0)
            assert e.steps[0][4] in d0
    if case.form == "dict" and max(case.counts) > 64:
        assert any(st[4] >= 1 << 17 for e in exp for st in e.steps), "no dict id beyond 2^17 was coded"
    if case.policy == "none":
        assert all(st[0] == case.counts[s] for s, e in enumerate(exp) for st in e.steps)
