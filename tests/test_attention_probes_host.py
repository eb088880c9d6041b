"""CPU: the position probes of tests/test_gpu_attention_probes.py see what the N(0, 1) reference tests cannot.

No kernel runs here.  On the probe inputs the fp64 reference is compared with five deliberately WRONG variants of
itself, each the result a kernel with one off-by-one would give:

* the first attended row dropped;
* row L0 taken from the stale cache instead of the new token;
* row L0 + 1 included;
* the window start one too early;
* one interior 32-row chunk-boundary row dropped.

Each must differ from the right result by more than 100 x the probe tests' tolerance at the probed pair, while on the
plain N(0, 1) inputs of the older tests at Lk = 1,100 the same variants move the typical (median) pair by LESS than
their flat 2e-3: the gap the probes close.  (Not every pair: the shift is about |v| e^s / (Lk sqrt(e)) for a lost key of
score s ~ N(0, 1), so roughly a third of the pairs move by 2e-3 to 1e-2 -- an error that touches every pair of a large
batch can trip the old bound, one that touches a few pairs, such as one wave's edge row, usually does not.)
"""

import pytest

torch = pytest.importorskip("torch")

from test_gpu_attention_probes import (attention_ref, build_case, build_seq_case, quant_torch,  # noqa: E402
                                       reference_and_tolerance, seq_ref, to_fp8, tolerance)

B, H = 2, 4


def _variants(T0, L0, W):
    """name -> (probe position, rows of the wrong variant, stale)."""
    s0 = max(0, L0 + 1 - W) if W else 0
    right = list(range(s0, L0 + 1))
    mid = s0 + 32 * ((L0 - s0) // 64)  # an interior chunk-boundary row of the split
    assert s0 < mid < L0
    out = {"first row dropped": (s0, right[1:], False),
           "stale row L0": (L0, right, True),
           "row L0 + 1 included": (L0 - 1, right + [L0 + 1], False),
           "chunk-boundary row dropped": (mid, [r for r in right if r != mid], False)}
    if s0 > 0:
        out["window start one too early"] = (L0 - 1, [s0 - 1] + right, False)
    return out


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0,L0,W", [(0, 1099, 0), (32, 1099, 0), (32, 300, 290), (32, 600, 300), (5, 1100, 1030)])
def test_probes_expose_off_by_one_variants(kv, T0, L0, W):
    for name, (j, rows, stale) in _variants(T0, L0, W).items():
        c = build_case(B, H, T0, L0, [[j] * H] * B, window=W, seed=L0 + W)
        if kv == "fp8":
            to_fp8(c, quant_torch)
        want, tol = reference_and_tolerance(c)
        wrong, _ = attention_ref(c, torch.float64, rows=rows, stale=stale)
        # every pair is probed at j (a shared prefix row keeps its first claimant; the others moved to L0)
        hit = (c.pos == j)
        if name == "window start one too early" and rows[0] < T0:  # a shared prefix row holds one stream's poison
            owner = (rows[0] * 7 + torch.arange(H)) % B
            hit &= torch.arange(B)[:, None] == owner[None, :]
        assert bool(hit.any())
        margin = ((wrong - want).abs() / tol).amax(-1)
        assert float(margin[hit].min()) > 100.0, (name, float(margin[hit].min()))


@pytest.mark.parametrize("T0,W", [(0, 0), (32, 0), (5, 1030)])
def test_plain_inputs_hide_the_same_variants(T0, W):
    """N(0, 1) q/k/v at Lk = 1,100 (what the older reference tests use): every wrong variant that loses or gains ONE
    row leaves the median pair (of 32) inside their 2e-3; the stale row L0 is two rows' worth (the right one lost, a
    wrong one gained), so twice that -- against ~1 to ~100 on the probe inputs."""
    L0, Bp, Hp = 1099, 4, 8
    for name, (j, rows, stale) in _variants(T0, L0, W).items():
        c = build_case(Bp, Hp, T0, L0, [[j] * Hp] * Bp, window=W, seed=L0 + W, probe=False)
        want, _ = attention_ref(c, torch.float64)
        wrong, _ = attention_ref(c, torch.float64, rows=rows, stale=stale)
        per_pair = (wrong - want).abs().amax(-1).flatten()
        print(f"{name}: median {float(per_pair.median()):.2e} max {float(per_pair.max()):.2e}")
        assert float(per_pair.median()) < (4e-3 if stale else 2e-3), (name, float(per_pair.median()))


def test_seq_probes_expose_a_leaking_future_row():
    """Sequence attention: letting row j* see key j* + 1 (a causal mask one too wide) moves the probed row by far
    more than 100 x tol; dropping the diagonal key does too."""
    Bs, T, Hs = 2, 200, 8
    qkv, jstar = build_seq_case(Bs, T, Hs, seed=5)
    want, pv, vmax = seq_ref(qkv, Bs, T, Hs, torch.float64)
    ref32, _, _ = seq_ref(qkv, Bs, T, Hs, torch.float32)
    tol = (tolerance(want, ref32, vmax) + 2.0 ** -10 * pv).view(Bs, T, Hs, 64)
    x = qkv.double().view(Bs, T, 3, Hs, 64)
    for b in range(Bs):
        for h in range(Hs):
            j = int(jstar[b, h])
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            for lo, hi in ((0, j + 2), (0, j)):  # one row too many / the diagonal dropped
                if hi > T or hi == 0:
                    continue
                p = torch.softmax((k[lo:hi] @ q[j]) * 0.125, 0)
                wrong = p @ v[lo:hi]
                margin = ((wrong - want.view(Bs, T, Hs, 64)[b, j, h]).abs() / tol[b, j, h]).max()
                assert float(margin) > 100.0, (b, h, j, hi, float(margin))
