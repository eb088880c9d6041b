"""CPU side of the decode step's divergence suite (``tests/decode_diverge_cases.py``): for every case the oracle alone
shows that each bad-token class is what its name claims -- the step diverges and leaves the oracle state untouched,
(a) sits on a step with k' < k, (f) has a -inf logit, the controls decode -- and that the kept ids the oracle now
reports (``oracle.decode_step_kept``) equal a plain numpy ranking of the row.  These runs are the values
``tests/test_gpu_decode_diverge.py`` expects of ``ns_decode_step``.
"""

import numpy as np
import pytest

from oracle import oracle
from tests import coder_vocab_cases as cv
from tests import decode_diverge_cases as dd
from tests.decode_diverge_cases import B, CASES


def _configs():
    return sorted({(c.family, c.vocab, c.dtype) for c in CASES})


def test_table_holds_every_family_twice_and_no_native_library_at_import():
    assert len(CASES) == 2 * len(dd.CONFIGS) == 20 and len({c.id for c in CASES}) == len(CASES)
    assert {c.family for c in CASES} == {"single", "sample", "quality", "wide-lds", "wide-sweep"}
    assert all(c.seed == dd.DEFAULT_SEED or (c.family, c.vocab, c.dtype, c.variant) in dd.SEEDS for c in CASES)
    assert sorted(dd.nsteps(s) for s in range(B)) == [10, 10, 11, 12, 13, 14]
    assert set(dd.ASSIGN[0]) | set(dd.ASSIGN[1]) == set(dd.CLASSES)
    qs = dd.QUALITIES
    assert len(qs) == B and all(len({q[i] for q in qs}) == B for i in range(3)), "the streams differ in all three"


def test_every_family_takes_the_form_it_claims():
    """The geometry each family is named after, from ``coder_vocab_cases`` (the sample rule is the library's own)."""
    for c in CASES:
        wide = cv.is_wide(c.vocab, c.dtype, c.topk)
        assert wide == c.family.startswith("wide"), c.id
        if c.family == "sample":
            assert cv.sample_on(c.vocab, c.dtype, c.topk), c.id
        elif not wide:
            assert not cv.sample_on(c.vocab, c.dtype, c.topk), c.id
        assert c.ld % 64 == 0 and c.ld > c.vocab, f"{c.id}: no pad column"
        kmax = max(st.trace[0] for e in dd.expected(c) for st in e.steps)
        if c.family == "wide-lds":
            assert kmax <= dd.WIDE_LDS_KEYS, c.id
        if c.family == "wide-sweep":
            assert kmax > dd.WIDE_LDS_KEYS, f"{c.id}: no step beyond the LDS key budget"
    assert all(q[0] <= cv.SINGLE_PASS_MAX_TOPK["f32"] for q in dd.QUALITIES)


@pytest.mark.parametrize("config", _configs(), ids=["-".join(map(str, c)) for c in _configs()])
def test_every_class_occurs_in_every_configuration(config):
    got = [e.cls for c in CASES if (c.family, c.vocab, c.dtype) == config for e in dd.expected(c)]
    assert len(got) == 2 * B and set(got) == set(dd.CLASSES)


def test_every_family_trims_two_ranks_or_more_under_a_class_a_token():
    """k - k' >= 2 on some class-a step of every family: an export loop that ran to k instead of k' then writes an
    id beyond the terminator's slot, where only the sentinel may be (with k - k' = 1 it would write the slot itself,
    which the terminator overwrites)."""
    for family in sorted({c.family for c in CASES}):
        gaps = [e.steps[e.bad_step].trace[0] - e.steps[e.bad_step].trace[1]
                for c in CASES if c.family == family for e in dd.expected(c) if e.cls == "a"]
        assert max(gaps) >= 2, family


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_oracle_run_and_bad_token_claims(case):
    exp = dd.expected(case)
    assert len(exp) == B
    nvalid = cv.nvalid(case.vocab, case.banned)
    for s, e in enumerate(exp):
        topk, temp, precision = case.quality(s)
        T = dd.nsteps(s)
        assert len(e.tokens) == len(e.steps) == T and e.cls == dd.class_of(case, s)
        assert e.steps[0].state == (0, 1 << precision, 0, 0) and e.final[3] == T
        assert len(e.decoded) == e.final[2] > 0
        assert 0 <= e.bad_step < T and e.bad_token != e.tokens[e.bad_step]
        for t, st in enumerate(e.steps):
            k, kp, sel, n, tok = st.trace
            assert 2 <= kp <= k <= min(topk, nvalid) and 0 <= sel < kp and tok == e.tokens[t] == st.kept[sel]
            # the oracle's kept ids against plain numpy: the non-banned ids by (value desc, id asc), first k'
            order = dd.numpy_order(dd.case_row(case, s, t), case.banned)
            assert len(order) == nvalid
            assert list(st.kept) == order[:kp].tolist(), f"stream {s} step {t}: kept ids differ from numpy's ranking"
        bt = e.bad_step
        k, kp = e.steps[bt].trace[:2]
        row = dd.case_row(case, s, bt)
        order = dd.numpy_order(row, case.banned).tolist()
        if e.cls == "a":
            assert kp < k and e.bad_token == order[kp]
        elif e.cls == "b":
            assert k < nvalid and e.bad_token == order[k]
        elif e.cls == "c":
            assert kp < nvalid and e.bad_token == order[-1] and e.bad_token not in case.banned
        elif e.cls == "g":
            assert bt == T - 1 and e.bad_token == order[k]
        elif e.cls == "f":
            assert bt == dd.MASK_STEP and row[e.bad_token] == -np.inf and e.bad_token not in case.banned
            assert int(np.isfinite(row.astype(np.float32)).sum()) == dd.MASK_FINITE
        else:
            want = {"d628": 628, "dV1": case.vocab - 1, "e-1": -1, "eV": case.vocab, "eld": case.ld - 1}[e.cls]
            assert e.bad_token == want and (e.cls[0] == "d") == (want in case.banned)
            assert e.cls != "eld" or case.vocab <= want < case.ld
        assert e.bad_token not in e.steps[bt].kept
        # the bad token diverges and leaves the oracle's state and bytes alone; the kept ids are still reported
        rc, after, tr, kept, out = dd.oracle_try(case, s, bt, e.bad_token)
        assert rc == oracle.OR_ERR_DIVERGE and after == e.steps[bt].state
        assert tr == (k, kp, -1, -1, -1) and tuple(kept) == e.steps[bt].kept
        assert out == (e.steps[bt - 1].out if bt else bytes(dd.out_bytes(case)))
        # the controls decode: rank k' - 1 and rank 0
        assert e.controls == (order[kp - 1], order[0])
        for rank, tok in zip((kp - 1, 0), e.controls):
            rc, after, tr, kept, _ = dd.oracle_try(case, s, bt, tok)
            assert rc == oracle.OR_OK and tr[2] == rank and tr[4] == tok and after[3] == bt + 1
            assert tuple(kept) == e.steps[bt].kept
