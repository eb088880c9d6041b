"""CPU side of the coder's vocabulary-size suite (``tests/coder_vocab_cases.py``): the geometry classes the case ids
claim are recomputed from V, the sample rule is read from the library (``ns_stream_quality_fill``, pure host
arithmetic), and every case runs through the oracle alone -- the values ``tests/test_gpu_coder_vocab.py`` expects of
the HIP coder.
"""

import pytest

from neuralsteganography_amd import _lib
from tests import coder_vocab_cases as cv
from tests.coder_vocab_cases import CASES, geometry, is_wide, sample_on


def _single(pred):
    """(V, dtype, topk) of the single-pass cases with the sample ON whose geometry satisfies ``pred``."""
    return [(c.vocab, c.dtype, c.topk) for c in CASES
            if sample_on(c.vocab, c.dtype, c.topk) and pred(c, geometry(c.vocab, c.dtype))]


def test_table_is_the_full_product_minus_the_refused_wide_cases():
    assert len(cv.VOCABS) == 18 and len(cv.CONFIGS) == 7
    assert len(CASES) == 18 * 7 - 2 and len({c.id for c in CASES}) == len(CASES)
    assert cv.UNSUPPORTED_WIDE == [(151936, "f32", 16, 50000), (151936, "f16", 22, 2000)]
    assert len({c for c in CASES if c.vocab == 151936}) == 5  # every single-pass row runs there
    assert all(c.seed == cv.DEFAULT_SEED or (c.vocab, c.dtype, c.topk) in cv.SEEDS for c in CASES)


def test_the_library_limits_the_ids_assume():
    assert _lib.max_topk(_lib.NS_DTYPE_F32) == 768 and _lib.max_topk(_lib.NS_DTYPE_F16) == 512
    assert {d: _lib.max_topk(cv.dtype_code(d)) for d in ("f32", "f16")} == cv.SINGLE_PASS_MAX_TOPK
    assert _lib.NS_MAX_BANNED >= 7
    # the sample is off below 8192 whatever the top-k, on at 8192 for a small one, off again beyond the Poisson bound
    assert cv.spec_j(8191, 2) == 0 and cv.spec_j(8191, 100) == 0
    assert cv.spec_j(8192, 100) > 0 and cv.spec_j(12288, 100) > 0 and cv.spec_j(12288, 300) > 0
    assert cv.spec_j(8192, 300) == 0, "K = 300 at V = 8192 (lambda = 150): the Poisson bound exceeds 160"
    assert cv.spec_j(8192, 768) == 0 and cv.spec_j(8192, 512) == 0


@pytest.mark.parametrize("vocab,dtype,ntiles,space,rem,last", [
    (65, "f32", 1, 0, 1, 65), (257, "f32", 2, 0, 2, 1), (515, "f16", 2, 0, 2, 3), (771, "f32", 4, 0, 4, 3),
    (8191, "f32", 32, 2, 0, 255), (8192, "f32", 32, 2, 0, 256), (8192, "f16", 16, 2, 0, 512),
    (8193, "f32", 33, 2, 1, 1), (8193, "f16", 17, 2, 1, 1), (12288, "f32", 48, 3, 0, 256), (12288, "f16", 24, 3, 0, 512),
    (15871, "f16", 31, 3, 7, 511), (16127, "f32", 63, 3, 15, 255), (16127, "f16", 32, 4, 0, 255),
    (50257, "f32", 197, 12, 5, 81), (50257, "f16", 99, 12, 3, 81)])
def test_geometry_of_the_named_vocabularies(vocab, dtype, ntiles, space, rem, last):
    g = geometry(vocab, dtype)
    assert (g.ts, g.nsamp) == ((512, 8) if dtype == "f16" else (256, 16))
    assert (g.ntiles, g.space, g.rem, g.last) == (ntiles, space, rem, last)
    assert g.nsamp * g.space + g.rem == g.ntiles and (g.ntiles - 1) * g.ts + g.last == vocab


def test_cases_cover_every_single_pass_geometry_class_with_the_sample_on():
    classes = {
        "space == 2": lambda c, g: g.space == 2,
        "remainder 0": lambda c, g: g.rem == 0,
        "remainder NSAMP - 1": lambda c, g: g.rem == g.nsamp - 1,
        "one-id last tile": lambda c, g: g.last == 1,
        "V % 64 == 0 (no pad)": lambda c, g: c.vocab % 64 == 0,
        "partial last tile that is a sample tile": lambda c, g: g.rem == 0 and g.last < g.ts,
        "ids beyond 65535": lambda c, g: c.vocab > 65536,
    }
    for name, pred in classes.items():
        hit = _single(pred)
        assert hit, f"no sample-on case covers: {name}"
        for dtype in ("f32", "f16"):  # both tile sizes reach every class
            assert any(h[1] == dtype for h in hit), f"no sample-on {dtype} case covers: {name}"
    # the named cases are where the ids say they are
    assert (8192, "f32", 100) in _single(lambda c, g: g.space == 2 and g.rem == 0 and c.vocab % 64 == 0)
    assert (8192, "f16", 100) in _single(lambda c, g: g.space == 2 and g.rem == 0 and c.vocab % 64 == 0)
    assert (8193, "f32", 100) in _single(lambda c, g: g.last == 1 and g.rem == 1)
    assert (12288, "f32", 300) in _single(lambda c, g: g.space == 3 and g.rem == 0)
    assert (15871, "f16", 100) in _single(lambda c, g: g.rem == 7 and g.last < g.ts)
    assert (16127, "f32", 300) in _single(lambda c, g: g.rem == 15)
    # topk 300 switches the sample off from 8192 up to (not including) 12288: only the topk-100 rows keep it on
    assert not sample_on(8192, "f32", 300) and not sample_on(8193, "f32", 300) and sample_on(8192, "f32", 100)
    # the sample needs space >= 2: no sample-on case below it
    assert not _single(lambda c, g: g.space < 2)


def test_cases_cover_the_sample_off_and_wide_classes():
    off = [c for c in CASES if not is_wide(c.vocab, c.dtype, c.topk) and not sample_on(c.vocab, c.dtype, c.topk)]
    assert {c.vocab for c in off} >= {65, 257, 515, 771, 1025, 4096, 8191}, "sample off: small vocabularies"
    assert any(c.vocab == 8192 and c.topk == 300 for c in off), "sample off by the Poisson bound at V >= 8192"
    assert any(geometry(c.vocab, c.dtype).ntiles == 1 for c in off), "fewer than one tile"
    assert any(c.topk > cv.nvalid(c.vocab, c.banned) for c in off), "K clamps to the valid ids"
    wide = [c for c in CASES if is_wide(c.vocab, c.dtype, c.topk)]
    # (id 628 lies outside a 515-id row: one banned id there, two at 771)
    assert min(c.vocab for c in wide if c.dtype == "f16") == 515 and cv.nvalid(515, [514, 628]) == 514 > 512
    assert min(c.vocab for c in wide if c.dtype == "f32") == 771 and cv.nvalid(771, [770, 628]) == 769 > 768
    assert not is_wide(770, "f32", 50000)
    for dtype in ("f32", "f16"):
        w = [c for c in wide if c.dtype == dtype]
        assert any(geometry(c.vocab, dtype).ntiles < cv.WIDE_WAVES for c in w), "wide: waves with empty slices"
        assert any(geometry(c.vocab, dtype).ntiles % cv.WIDE_WAVES for c in w), "wide: a short last slice"
        assert any(c.vocab > 65536 for c in w), "wide: ids beyond 16 bits"
        assert any(c.vocab == cv.WIDE_MAX_VOCAB for c in w), "wide: the 17-bit id limit"
    assert geometry(771, "f32").ntiles == 4 and geometry(515, "f16").ntiles == 2
    assert all(c.vocab <= cv.WIDE_MAX_VOCAB for c in wide)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_oracle_completes_every_stream(case):
    """The oracle alone: every step OR_OK (``oracle_stream`` raises otherwise), no stall, and its own decode gives
    the payload back."""
    exp = cv.expected(case)
    assert len(exp) == cv.B
    for s, e in enumerate(exp):
        assert e.bits == cv.payload_bits(s) and len(e.bits) == 48 - 5 * s
        assert 1 <= len(e.tokens) == len(e.traces) <= cv.MAX_STEPS
        assert all(0 <= t < case.vocab and t not in case.banned for t in e.tokens)
        assert e.decoded[: len(e.bits)] == e.bits, f"stream {s}: the oracle's decode differs from the payload"
        assert all(tr[0] <= min(case.topk, cv.nvalid(case.vocab, case.banned)) for tr in e.traces)
