"""Inputs and expected values for the fp8 KV-cache value tests (tests/test_fp8_cases_host.py on the CPU,
tests/test_gpu_fp8_values.py on the GPU).  Pure numpy / torch: no GPU and no native library is touched here.

The fp8 cache stores OCP e4m3fn bytes: sign, 4 exponent bits (bias 7), 3 mantissa bits; no infinity; the one NaN code
per sign is S.1111.111 (0x7F / 0xFF); the largest finite value is S.1111.110 = 1.75 * 2^8 = 448.  A byte's magnitude
code c = byte & 0x7F is worth

    c < 8 : c * 2^-9                        (subnormals, the first one 2^-9)
    c >= 8: (8 + (c & 7)) * 2^((c >> 3) - 10)

and the codes are ordered like the values, so a conversion is "the nearest code, ties to the even code, saturated at
0x7E".  ``e4m3fn_from_f16_bits`` does exactly that on the integer fields of the fp16 pattern, ``f64_from_e4m3fn`` is
its inverse; neither calls torch.  The ``variant`` argument gives the deliberately WRONG conversions the host test uses
to show that the GPU checks would notice them.
"""

import numpy as np
import torch

D = 64
NAN_CODE, MAX_CODE = 0x7F, 0x7E
VARIANTS = ("nan_as_-448", "sat240", "truncate")


# ------------------------------------------------------------------------------------- from-spec integer reference
def e4m3fn_from_f16_bits(bits, variant=None):
    """uint16 fp16 bit patterns -> uint8 e4m3fn bytes: round to nearest even, finite values and +-inf saturate to
    +-448 (0x7E / 0xFE), -0 -> 0x80, NaN -> the NaN byte of its sign."""
    assert variant is None or variant in VARIANTS
    bits = np.asarray(bits, dtype=np.uint16)
    b = bits.astype(np.int64)
    sign = (b >> 15) << 7
    e, m = (b >> 10) & 31, b & 1023
    # |x| as an integer count of 2^-24 (the fp16 subnormal unit); below 2^41
    mag = np.where(e == 0, m, (1024 + m) << np.maximum(e - 1, 0))
    nbits = np.frexp(mag.astype(np.float64))[1].astype(np.int64)  # bit length (exact: mag < 2^53); 0 for 0
    # e4m3 exponent field of the binade |x| lies in (1 for the subnormal range); one code step there is 2^(E - 10),
    # i.e. 2^(E + 14) units of 2^-24
    E = np.maximum(nbits - 1 - 24 + 7, 1)
    sh = E + 14
    q, rem, half = mag >> sh, mag & ((1 << sh) - 1), 1 << (sh - 1)
    if variant != "truncate":
        q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # q in [0, 16]: 8 .. 15 the binade's codes, 16 the next binade's first code, below 8 a subnormal (E = 1)
    code = np.minimum(((E - 1) << 3) + q, 0x77 if variant == "sat240" else MAX_CODE)
    inf, nan = (e == 31) & (m == 0), (e == 31) & (m != 0)
    code = np.where(inf, 0x77 if variant == "sat240" else MAX_CODE, code)
    out = np.where(nan, sign | NAN_CODE, sign | code)
    if variant == "nan_as_-448":
        out = np.where(nan, 0x80 | MAX_CODE, out)
    return out.astype(np.uint8)


def f64_from_e4m3fn(byte):
    """uint8 e4m3fn bytes -> float64 values (NaN for 0x7F / 0xFF; 0x80 is -0.0)."""
    b = np.asarray(byte, dtype=np.uint8).astype(np.int64)
    c = b & 0x7F
    mag = np.where(c < 8, np.ldexp(c.astype(np.float64), -9), np.ldexp((8 + (c & 7)).astype(np.float64), (c >> 3) - 10))
    mag = np.where(c == NAN_CODE, np.nan, mag)
    return np.where(b >> 7 == 1, -mag, mag)


def is_nan_byte(byte):
    return (np.asarray(byte) & 0x7F) == NAN_CODE


def f16_bits_of(x):
    """float values (exactly representable in fp16) -> their uint16 patterns."""
    return np.asarray(x, dtype=np.float16).view(np.uint16)


def f16_tensor(bits, device="cpu"):
    """uint16 patterns -> a torch fp16 tensor of the same shape with exactly these bits (NaN payloads kept)."""
    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16)).to(device).view(torch.float16)


def byte_tensor(byte, device="cpu"):
    return torch.from_numpy(np.array(byte, dtype=np.uint8)).to(device)


# --------------------------------------------------------------------------------------- (a) every fp16 pattern
def all_f16_patterns():
    return np.arange(65536, dtype=np.uint16)


def nonfinite_mask(bits):
    return ((np.asarray(bits) >> 10) & 31) == 31  # 2 infinities and 2,046 NaNs among the 65,536 patterns


def quantiser_case():
    """(bits [5 * 65536], expected bytes): every pattern in natural order, rotated by 1, 2 and 3 (so each pattern sits
    at each of the 4 positions of a packed word, next to three different neighbours) and once shuffled."""
    p = all_f16_patterns()
    bits = np.concatenate([p, np.roll(p, 1), np.roll(p, 2), np.roll(p, 3), np.random.default_rng(8).permutation(p)])
    return bits, e4m3fn_from_f16_bits(bits)


# ----------------------------------------------------------------------- (b) every pattern through the append sites
N_FINITE_ROWS, N_ROWS = 992, 1024  # rows of 64 values: 63,488 finite patterns, then the 2,048 non-finite ones


def append_site_rows():
    """(k_bits, v_bits) uint16 [1024, 64]: both hold every fp16 pattern once, the finite ones in rows 0 .. 991 and the
    non-finite ones in rows 992 .. 1023 (so that they can live in streams or sequences of their own); k in ascending
    order, v shuffled, so a row of v is no copy of a row of k and a pattern meets other neighbours in its word."""
    p = all_f16_patterns()
    nf = nonfinite_mask(p)
    k = np.concatenate([p[~nf], p[nf]])
    rng = np.random.default_rng(88)
    v = np.concatenate([rng.permutation(p[~nf]), rng.permutation(p[nf])])
    return k.reshape(N_ROWS, D), v.reshape(N_ROWS, D)


def append_site_qkv(n_tokens, H, seed=0):
    """qkv [n_tokens, 3 H D] as fp16 bit patterns: q ~ N(0, 1); token t, head h takes row (t * H + h) mod 1024 of
    ``append_site_rows`` as its k and its v.  With n_tokens * H >= 1024 every pattern passes through k and through v;
    tokens from 992 / H on (up to 1024 / H) are the non-finite ones.  Returns (qkv_bits, k_rows, v_rows), the rows as
    [n_tokens, H, 64] patterns."""
    assert N_FINITE_ROWS % H == 0 and N_ROWS % H == 0
    kb, vb = append_site_rows()
    idx = (np.arange(n_tokens * H) % N_ROWS).reshape(n_tokens, H)
    q = torch.randn((n_tokens, H, D), generator=torch.Generator().manual_seed(seed)).half().numpy().view(np.uint16)
    k, v = kb[idx], vb[idx]
    return np.concatenate([q.reshape(n_tokens, -1), k.reshape(n_tokens, -1), v.reshape(n_tokens, -1)], axis=1), k, v


def nonfinite_tokens(n_tokens, H):
    """bool [n_tokens]: the tokens of ``append_site_qkv`` that carry non-finite patterns."""
    idx = (np.arange(n_tokens * H) % N_ROWS).reshape(n_tokens, H)
    return (idx >= N_FINITE_ROWS).any(axis=1)


# ------------------------------------------------------------------------------ (c) V dequantiser: Latin arrangement
def _unit(n, d, value):
    x = np.zeros((n, D), dtype=np.float64)
    x[:, d] = value
    return x


def v_sweep_case(n_pairs, T0=0):
    """One cached row per pair plus the new token, scale = 1: q = 4 e0, cached k = +8 e0, new k = -8 e0, new v = 0, so
    the cached row's softmax weight is 1 / (1 + e^-64 ...) = 1.0f exactly and the output is the cached v row,
    dequantised.  Pair p holds byte (p + d) mod 256 at dim d: 256 pairs cover every (byte, dim).  T0 > 0 adds a shared
    prefix of T0 rows k = -8 e0, v = 0 (weight e^-64 each, as the new token).

    Returns dict(q, k_new, v_new: fp16 patterns [n_pairs, 64]; k_row, v_row: cached bytes [n_pairs, 64];
    k_pre, v_pre: prefix bytes [64]; want: float64 [n_pairs, 64], NaN where the byte is a NaN byte)."""
    p = np.arange(n_pairs)[:, None]
    v_row = ((p + np.arange(D)[None, :]) % 256).astype(np.uint8)
    plus8 = e4m3fn_from_f16_bits(f16_bits_of(_unit(n_pairs, 0, 8.0)))
    minus8 = e4m3fn_from_f16_bits(f16_bits_of(_unit(1, 0, -8.0)))[0]
    assert f64_from_e4m3fn(plus8[0, 0]) == 8.0 and f64_from_e4m3fn(minus8[0]) == -8.0
    return dict(q=f16_bits_of(_unit(n_pairs, 0, 4.0)), k_new=f16_bits_of(_unit(n_pairs, 0, -8.0)),
                v_new=np.zeros((n_pairs, D), dtype=np.uint16), k_row=plus8, v_row=v_row, k_pre=minus8,
                v_pre=np.zeros(D, dtype=np.uint8), want=f64_from_e4m3fn(v_row), T0=T0, scale=1.0)


def v_sweep_formula_f32(case):
    """The reference formula of the V sweep evaluated in float32 (softmax over [prefix rows, cached row, new token]
    times the dequantised v rows): the host test checks that it returns deq(byte) bit for bit."""
    n, T0 = case["q"].shape[0], case["T0"]
    q = f16_tensor(case["q"]).float()
    deq = lambda b: torch.from_numpy(f64_from_e4m3fn(b)).float()  # noqa: E731
    k_new = deq(e4m3fn_from_f16_bits(case["k_new"]))
    rows_k = [deq(case["k_pre"])[None, :].expand(n, -1)] * T0 + [deq(case["k_row"]), k_new]
    rows_v = [deq(case["v_pre"])[None, :].expand(n, -1)] * T0 + [deq(case["v_row"]), torch.zeros(n, D)]
    s = torch.stack([(q * k).sum(-1) for k in rows_k], dim=1) * np.float32(case["scale"])
    w = torch.softmax(s, dim=1)
    out = torch.zeros(n, D)
    for j, v in enumerate(rows_v):
        out = out + w[:, j:j + 1] * v
    return out


# ---------------------------------------------------------------------------------- (d) K dequantiser: one-hot rows
K_TOL = 2.0 ** -10
# The output is sigmoid(c * deq) in (0, 1): its fp16 half-ulp is at most 2^-12 and the fp32 exp2 / division error is
# ~1e-6, so 2^-10 is four times the rounding; nothing here is measured on the kernel.


def k_sweep_scale(byte):
    """c = 2^-floor(log2 |deq(byte)|) (512 for the zero bytes, 1 for the NaN bytes): c * |deq| lies in [1, 2)."""
    val = np.abs(f64_from_e4m3fn(byte))
    ok = np.isfinite(val) & (val > 0)
    ex = np.floor(np.log2(np.where(ok, val, 1.0)))
    c = np.ldexp(1.0, (-ex).astype(np.int64))
    return np.where(val == 0, 512.0, np.where(ok, c, 1.0))


def k_sweep_case(H, T0=0, pre_dim=None):
    """Every byte (the two NaN bytes last) at every head dim: pair i = byte_index * 64 + d.  Cached k row: the byte at
    dim d, 0 elsewhere; q = c e_d; cached v = e0; new k = 0, new v = 0; scale = 1.  Output[0] = sigmoid(c deq(byte)).

    T0 > 0: the shared prefix of head h is k = -448 e_x, v = 0 with x = pre_dim[h], and q gets 1 at dim x: the prefix
    rows score -448 (weight exactly 0 in fp32) and the cached row's score is unchanged (its byte at x is 0), provided
    no pair of head h tests dim x -- pair i sits on head i mod H, i.e. on head d mod H for even H.

    Returns dict(byte [n], dim [n], q, k_new, v_new: fp16 patterns [n, 64]; k_row, v_row: bytes [n, 64];
    k_pre, v_pre: bytes [H, 64]; want: float64 [n] (NaN for the NaN bytes))."""
    assert D % H == 0
    finite = np.array([b for b in range(256) if b & 0x7F != NAN_CODE], dtype=np.uint8)
    order = np.concatenate([finite, np.array([0x7F, 0xFF], dtype=np.uint8)])
    byte = np.repeat(order, D)
    dim = np.tile(np.arange(D), 256)
    n = byte.size
    c = k_sweep_scale(byte)
    q = np.zeros((n, D))
    q[np.arange(n), dim] = c
    k_row = np.zeros((n, D), dtype=np.uint8)
    k_row[np.arange(n), dim] = byte
    one = e4m3fn_from_f16_bits(f16_bits_of(1.0))
    v_row = np.zeros((n, D), dtype=np.uint8)
    v_row[:, 0] = one
    k_pre = np.zeros((H, D), dtype=np.uint8)
    if T0 > 0:
        pre_dim = np.asarray(pre_dim)
        head = np.arange(n) % H
        assert not (dim == pre_dim[head]).any()
        q[np.arange(n), pre_dim[head]] = 1.0
        k_pre[np.arange(H), pre_dim] = 0x80 | MAX_CODE
    want = 1.0 / (1.0 + np.exp(-c * f64_from_e4m3fn(byte)))
    return dict(byte=byte, dim=dim, q=f16_bits_of(q), k_new=np.zeros((n, D), dtype=np.uint16),
                v_new=np.zeros((n, D), dtype=np.uint16), k_row=k_row, v_row=v_row, k_pre=k_pre,
                v_pre=np.zeros((H, D), dtype=np.uint8), want=want, T0=T0, scale=1.0)


def k_sweep_output(byte, deq=f64_from_e4m3fn):
    """sigmoid(c(byte) * deq(byte)): what output[0] of the K sweep is with the dequantiser ``deq``."""
    return 1.0 / (1.0 + np.exp(-k_sweep_scale(byte) * deq(byte)))


def deq_one_code_off(byte, exponent_field=9):
    """A dequantiser that is one code off (reads code c as c + 1) in the binade with this exponent field only."""
    b = np.asarray(byte, dtype=np.uint8)
    hit = ((b >> 3) & 15) == exponent_field
    return f64_from_e4m3fn(np.where(hit, b + 1, b).astype(np.uint8))


# ------------------------------------------------------------------------------------------- (e) heavy-tailed K / V
HEAVY_K = {5: 24.0, 41: 24.0, 18: 200.0}  # head dim -> factor: outlier dimensions as trained GPT-2 keys have them
HEAVY_V = {7: 24.0, 50: 200.0}
HEAVY_SHAPES = [(3, 2, 0, 40), (3, 2, 32, 300), (2, 2, 7, 1099)]  # (B, H, T0, L0) of the host-side margins


def heavy_tail(c):
    """Scale the K and V of a ``build_case(probe=False)`` case (tests/test_gpu_attention_probes.py) per head dim, in
    place: cached rows, prefix rows and the new token's k / v alike.  N(0, 1) * 200 reaches past 448 for ~2.5 % of the
    entries of that dim, so the saturation edge, the 16 .. 448 binades and the bulk all occur in one softmax."""
    x = c.qkv.view(c.B, 3, c.H, D)
    for d, f in HEAVY_K.items():
        for t in (c.kp, c.ks, x[:, 1]):
            t[..., d] *= f
    for d, f in HEAVY_V.items():
        for t in (c.vp, c.vs, x[:, 2]):
            t[..., d] *= f
    return c


def quantiser(variant=None):
    """fp16 tensor -> uint8 tensor through the integer reference (or one of its wrong variants), on the CPU."""
    def quant(t):
        bits = t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
        return torch.from_numpy(e4m3fn_from_f16_bits(bits, variant)).to(t.device)
    return quant


def random_finite_bytes(shape, generator, device="cpu"):
    """Uniformly random bytes without the two NaN codes: magnitudes log-uniform from 2^-9 to 448."""
    b = torch.randint(0, 254, shape, generator=generator, device=device, dtype=torch.int16)
    return (b + (b >= 0x7F).to(torch.int16)).to(torch.uint8)  # 0 .. 0x7E and 0x80 .. 0xFE
