"""CPU: the reference and the inputs of tests/test_gpu_fp8_values.py are sound, and its bars would catch a wrong kernel.

No kernel runs here.  Three things are checked:

* the from-spec integer e4m3fn conversion of tests/fp8_cases.py against torch's CPU cast on all 65,536 fp16 patterns,
  and its inverse against torch on all 256 bytes;
* that the byte sweeps are well conditioned: the V sweep's reference formula gives deq(byte) bit for bit in float32 (so
  exact equality is a fair bar), and in the K sweep a neighbouring byte moves the output by >= 10 x the tolerance;
* that deliberately WRONG conversions -- NaN stored as -448, saturation at 240 (the fnuz maximum), truncation instead of
  round-to-nearest-even, a dequantiser one code off in one binade -- miss those bars by a wide margin at every pattern,
  byte or (stream, head) pair they touch, the heavy-tailed attention case included.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fp8_cases as fc  # noqa: E402
from test_gpu_attention_probes import attention_ref, build_case, to_fp8, tolerance  # noqa: E402

PATTERNS = fc.all_f16_patterns()
ISNAN = np.isnan(PATTERNS.view(np.float16))


def _torch_quant(bits):
    return fc.f16_tensor(bits).float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------ reference against torch
def test_integer_reference_equals_torch_on_every_fp16_pattern():
    got, want = fc.e4m3fn_from_f16_bits(PATTERNS), _torch_quant(PATTERNS)
    assert ISNAN.sum() == 2046
    assert np.array_equal(got[~ISNAN], want[~ISNAN])
    assert fc.is_nan_byte(got[ISNAN]).all() and fc.is_nan_byte(want[ISNAN]).all()
    assert not fc.is_nan_byte(got[~ISNAN]).any()
    assert len(set(got.tolist())) == 256  # every byte is reached
    f = PATTERNS.view(np.float16)
    assert got[f == np.inf].tolist() == [0x7E] and got[f == -np.inf].tolist() == [0xFE]  # infinities saturate
    assert got[0x8000] == 0x80  # -0 keeps its sign
    assert (got[~ISNAN] >> 7 == PATTERNS[~ISNAN] >> 15).all()  # ... as every value does, the ones rounded to 0 too


def test_inverse_equals_torch_on_every_byte():
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).double().numpy()
    got = fc.f64_from_e4m3fn(b)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isnan(got).sum() == 2 and np.nanmax(got) == 448.0 and np.nanmin(got) == -448.0
    # round trip: every non-NaN byte is the conversion of its own value (all exact in fp16)
    ok = ~np.isnan(got)
    assert np.array_equal(fc.e4m3fn_from_f16_bits(fc.f16_bits_of(got[ok])), b[ok])


def test_builders_cover_every_pattern_and_keep_non_finite_ones_apart():
    bits, want = fc.quantiser_case()
    for pos in range(4):  # every pattern at every position of a packed word
        assert len(set(bits[pos::4].tolist())) == 65536
    assert want.shape == bits.shape
    k, v = fc.append_site_rows()
    for rows in (k, v):
        assert sorted(rows.reshape(-1).tolist()) == list(range(65536))
        assert not fc.nonfinite_mask(rows[:fc.N_FINITE_ROWS]).any() and fc.nonfinite_mask(rows[fc.N_FINITE_ROWS:]).all()
    qkv, kr, vr = fc.append_site_qkv(520, 2)
    assert qkv.shape == (520, 3 * 2 * 64) and np.array_equal(kr[:512].reshape(1024, 64), k)
    bad = fc.nonfinite_tokens(520, 2)
    assert bad.sum() == 16 and bad[496:512].all()
    assert np.isfinite(fc.f16_tensor(qkv).float().numpy()[~bad]).all()


# ------------------------------------------------------------------------------- the sweeps are well conditioned
@pytest.mark.parametrize("T0", [0, 7, 32])
def test_v_sweep_formula_returns_the_byte_bit_for_bit_in_float32(T0):
    c = fc.v_sweep_case(256, T0)
    for d in range(64):  # the Latin arrangement: every byte at every dim
        assert sorted(c["v_row"][:, d].tolist()) == list(range(256))
    got = fc.v_sweep_formula_f32(c).numpy()
    want = c["want"].astype(np.float32)
    assert np.array_equal(got, want, equal_nan=True)  # exact equality on the GPU is a fair bar
    assert np.isnan(want).sum() == 2 * 64
    # ... and every value survives the fp16 output
    assert np.array_equal(want.astype(np.float16).astype(np.float32), want, equal_nan=True)


def test_k_sweep_moves_by_ten_tolerances_for_a_neighbouring_byte():
    c = fc.k_sweep_case(2)
    assert c["byte"].size == 256 * 64 and np.isnan(c["want"]).sum() == 2 * 64
    scale = fc.k_sweep_scale(np.arange(256, dtype=np.uint8))
    assert scale.min() == 2.0 ** -8 and scale.max() == 2.0 ** 9  # all exact in fp16
    s = (scale * fc.f64_from_e4m3fn(np.arange(256, dtype=np.uint8)))
    fin = ~fc.is_nan_byte(np.arange(256))
    assert ((np.abs(s[fin]) >= 1) & (np.abs(s[fin]) < 2) | (s[fin] == 0)).all()
    worst = np.inf
    for b in range(256):
        if b & 0x7F == 0x7F:
            continue
        for nb in (b - 1, b + 1):  # the neighbouring codes of the same sign, read with this byte's q
            if nb < 0 or nb > 255 or (nb ^ b) & 0x80 or nb & 0x7F == 0x7F:
                continue
            right = fc.k_sweep_output(np.uint8(b))
            wrong = 1.0 / (1.0 + np.exp(-scale[b] * fc.f64_from_e4m3fn(np.uint8(nb))))
            worst = min(worst, abs(float(right) - float(wrong)))
    print(f"K sweep: smallest output difference to a neighbouring byte {worst:.5f} = {worst / fc.K_TOL:.1f} x tol")
    assert worst >= 10 * fc.K_TOL


# ------------------------------------------------------------------- wrong conversions miss the GPU checks' bars
def test_nan_stored_as_minus_448_fails_the_quantiser_bar():
    """Check (a) asks for a NaN byte at every NaN pattern: the variant gives a finite byte at all 2,046 of them."""
    got = fc.e4m3fn_from_f16_bits(PATTERNS, "nan_as_-448")
    assert (got[ISNAN] == 0xFE).all() and not fc.is_nan_byte(got[ISNAN]).any()
    assert np.array_equal(got[~ISNAN], fc.e4m3fn_from_f16_bits(PATTERNS)[~ISNAN])


def test_saturation_at_240_fails_the_quantiser_bar():
    """Check (a) is bit equality: the variant differs at every pattern from 248 (the tie between 240 and 256, which
    goes to the even code 256) up, infinities included, by 16 or more after dequantisation -- and nowhere else."""
    right, got = fc.e4m3fn_from_f16_bits(PATTERNS), fc.e4m3fn_from_f16_bits(PATTERNS, "sat240")
    f = np.abs(PATTERNS.view(np.float16).astype(np.float64))
    touched = ~ISNAN & (f >= 248)
    assert np.array_equal(right != got, touched) and touched.sum() > 5000
    gap = np.abs(fc.f64_from_e4m3fn(right[touched]) - fc.f64_from_e4m3fn(got[touched]))
    assert gap.min() >= 16.0


def test_truncation_fails_the_quantiser_bar():
    """... and truncation is one whole code below round-to-nearest-even at every pattern above its code's midpoint
    (and at the ties of odd codes) that does not saturate: close to half of the patterns between 2^-10 and 448, some in
    every binade, each off by 1/16 of its value or more."""
    right, got = fc.e4m3fn_from_f16_bits(PATTERNS), fc.e4m3fn_from_f16_bits(PATTERNS, "truncate")
    diff = right != got
    assert not diff[ISNAN].any()
    f = np.abs(PATTERNS.view(np.float16).astype(np.float64))
    inside = ~ISNAN & (f > 2.0 ** -10) & (f < 448)
    assert not diff[~inside].any() and 0.45 * inside.sum() < diff.sum() < 0.55 * inside.sum()
    assert set(((right[diff] >> 3) & 15).tolist()) == set(range(16))
    assert ((right[diff] & 0x7F).astype(int) - (got[diff] & 0x7F).astype(int) == 1).all()
    a, b = fc.f64_from_e4m3fn(right[diff]), fc.f64_from_e4m3fn(got[diff])
    assert (np.abs(a - b) >= np.abs(a) / 16.0).all()


def test_dequantiser_one_code_off_fails_both_sweeps():
    """A dequantiser that reads one binade's codes one too high: the V sweep (exact equality) sees a whole code step,
    the K sweep (2^-10) at least 12 tolerances, at every byte of that binade."""
    b = np.arange(256, dtype=np.uint8)
    for ef in range(15):  # (the top binade holds the NaN code: its neighbour is not a value)
        off = fc.deq_one_code_off(b, ef)
        hit = ((b >> 3) & 15) == ef
        right = fc.f64_from_e4m3fn(b)
        assert np.array_equal(off[~hit], right[~hit], equal_nan=True)
        assert (np.abs(off[hit] - right[hit]) >= np.abs(right[hit]) / 15.0).all() and (off[hit] != right[hit]).all()
        moved = np.abs(fc.k_sweep_output(b[hit], lambda x: fc.deq_one_code_off(x, ef)) - fc.k_sweep_output(b[hit]))
        assert moved.min() >= 12 * fc.K_TOL, (ef, moved.min() / fc.K_TOL)


# ------------------------------------------------------------------------------------------- heavy-tailed attention
@pytest.mark.parametrize("B,H,T0,L0", fc.HEAVY_SHAPES)
def test_heavy_tailed_inputs_expose_saturation_and_truncation_at_every_pair(B, H, T0, L0):
    """On the inputs of check (e) -- N(0, 1) with outlier dimensions -- a cache saturated at 240 or truncated moves
    every (stream, head) pair by more than 10 x the unchanged probe tolerance.  The inputs are the builder's default
    seed.  Truncation touches every entry, so its margin (25 x and more) hardly depends on the draw; saturation at 240
    touches a pair only through the rows that carry its softmax weight, so over other seeds an occasional pair of
    these 6 + 6 + 4 stays inside the tolerance (seeds 0 .. 7: two of 128 pairs) -- at the GPU check's 1,104 pairs a
    kernel saturating at 240 meets hundreds of pairs it moves."""
    def case(variant):
        c = fc.heavy_tail(build_case(B, H, T0, L0, np.full((B, H), -1), seed=0, probe=False))
        return to_fp8(c, fc.quantiser(variant))

    c = case(None)
    want, vmax = attention_ref(c, torch.float64)
    ref32, _ = attention_ref(c, torch.float32)
    tol = tolerance(want, ref32, vmax)
    for variant in ("sat240", "truncate"):
        wrong, _ = attention_ref(case(variant), torch.float64)
        margin = ((wrong - want).abs() / tol).amax(-1)
        print(f"{variant} (B, H, T0, L0) = {(B, H, T0, L0)}: smallest margin over pairs {float(margin.min()):.1f}")
        assert float(margin.min()) > 10.0, (variant, float(margin.min()))
