"""GPU: the exported LM entry points that only whole-model runs reached (include/nsg_lm.h, csrc/nsg_lm.hip):
ns_lm_ln_gemm, ns_lm_embed_ln_rows, ns_lm_embed_seq_ln, ns_lm_layernorm_rows, the out-of-range token ids of
ns_lm_embed_ln and the layer norm's shape limits -- each against the two-kernel / one-row form it must equal bit for
bit and against a float64 torch reference within the tolerances test_gpu_lm_kernels.py already states
(GEMM: |err| <= 2e-3 |ref| + 2e-3; layer norm: |err| <= 2e-3 |ref| + 4e-3).
"""

import math

import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from test_gpu_lm_kernels import EPIS, _ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _ln64(x, w, b):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), EPS)


def _ln_close(got, want):
    return bool(((got.double() - want).abs() <= 2e-3 * want.abs() + 4e-3).all())


# ------------------------------------------------------------------------------------------------ ns_lm_ln_gemm
@pytest.mark.parametrize("N", [16, 2304, 8192])
@pytest.mark.parametrize("K", [64, 768, 1024, 1088])
def test_ln_gemm_equals_layernorm_then_gemm(K, N):
    """ns_lm_ln_gemm gives the bits of ns_lm_layernorm followed by ns_lm_gemm on the fused path (M <= 16, K <= 1024,
    N < 8192: the normalised rows d_a stay untouched) and off it, and both stages agree with float64."""
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(K + N)
    wt = (torch.randn((N, K), generator=g, device="cuda") / math.sqrt(K)).half()
    bias = (0.5 * torch.randn((N,), generator=g, device="cuda")).half()
    lw = torch.randn((K,), generator=g, device="cuda").half()
    lb = torch.randn((K,), generator=g, device="cuda").half()
    fused_cases = []
    for M in (1, 4, 15, 16, 17):
        x = (3 * torch.randn((M, K), generator=g, device="cuda") + 1).half()
        a2 = torch.empty((M, K), device="cuda").half()
        assert L.ns_lm_layernorm(x.data_ptr(), K, lw.data_ptr(), lb.data_ptr(), a2.data_ptr(), K, M, K, EPS,
                                 _stream_handle()) == 0
        assert _ln_close(a2, _ln64(x, lw, lb))
        for epi in ("store", "gelu", "residual", "f32"):
            ydt = torch.float32 if epi == "f32" else torch.float16
            y0 = torch.full((M + 1, N), 7.0, device="cuda").to(ydt)  # one guard row
            y0[:M] = torch.randn((M, N), generator=g, device="cuda").to(ydt) if epi == "residual" else float("nan")
            b = bias if (M + len(epi)) % 2 else None
            bp = b.data_ptr() if b is not None else None
            y2 = y0.clone()
            assert L.ns_lm_gemm(a2.data_ptr(), K, wt.data_ptr(), K, bp, y2.data_ptr(), N, M, N, K, EPIS[epi],
                                _stream_handle()) == 0
            y = y0.clone()
            a = torch.full((M, K), 5.0, device="cuda").half()
            assert L.ns_lm_ln_gemm(x.data_ptr(), K, lw.data_ptr(), lb.data_ptr(), EPS, wt.data_ptr(), K, bp,
                                   y.data_ptr(), N, M, N, K, EPIS[epi], a.data_ptr(), K, _stream_handle()) == 0
            torch.cuda.synchronize()
            assert torch.equal(y, y2), (M, epi)  # the guard row included
            assert torch.equal(y[M], y0[M])
            want = _ref(a2, wt, b, y0[:M], epi)
            err = (y[:M].double() - want).abs()
            assert bool((err <= 2e-3 * want.abs() + 2e-3).all()), (M, epi, float(err.max()))
            fused = bool((a == 5.0).all())
            assert fused or torch.equal(a, a2)
            assert fused == (M <= 16 and K <= 1024 and N < 8192), (M, K, N, epi)
            # without a buffer for the normalised rows only the fused path can run
            y = y0.clone()
            rc = L.ns_lm_ln_gemm(x.data_ptr(), K, lw.data_ptr(), lb.data_ptr(), EPS, wt.data_ptr(), K, bp, y.data_ptr(),
                                 N, M, N, K, EPIS[epi], None, 0, _stream_handle())
            torch.cuda.synchronize()
            if fused:
                assert rc == 0 and torch.equal(y, y2)
                fused_cases.append((M, epi))
            else:
                assert rc == _lib.NS_ERR_CONFIG
                assert torch.equal(y[M], y0[M]) and (epi == "residual" or bool(torch.isnan(y[:M]).all()))
    print(f"ns_lm_ln_gemm K={K} N={N}: fused for M in {sorted({m for m, _ in fused_cases})}")


# --------------------------------------------------------------------------------------- embedding + layer norm
def _embed_tables(V, P, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    wte = torch.randn((V, C), generator=g, device="cuda").half()
    wpe = torch.randn((P, C), generator=g, device="cuda").half()
    w = torch.randn((C,), generator=g, device="cuda").half()
    b = torch.randn((C,), generator=g, device="cuda").half()
    return g, wte, wpe, w, b


def _embed_one(tok, L, wte, wpe, w, b, V, P, C):
    """ns_lm_embed_ln on one row with the host-side length L."""
    t = torch.tensor([tok], dtype=torch.int32, device="cuda")
    h = torch.empty((1, C), device="cuda").half()
    a = torch.empty((1, C), device="cuda").half()
    assert _lib.lib().ns_lm_embed_ln(t.data_ptr(), wte.data_ptr(), wpe.data_ptr(), V, P, L, None, h.data_ptr(), C,
                                     w.data_ptr(), b.data_ptr(), a.data_ptr(), C, 1, C, EPS, _stream_handle()) == 0
    torch.cuda.synchronize()
    return h[0], a[0]


def test_embed_ln_rows_takes_each_rows_own_position():
    V, P, C = 1000, 64, 256
    g, wte, wpe, w, b = _embed_tables(V, P, C, seed=21)
    lens_l = [0, P - 1, P, 2 * P + 3, 5, 1, P + 1, 3 * P - 1, 17]  # the position wraps modulo n_positions
    M = len(lens_l)
    lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
    tok = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
    h = torch.full((M + 1, C), 7.0, device="cuda").half()
    a = torch.full((M + 1, C), 7.0, device="cuda").half()
    assert _lib.lib().ns_lm_embed_ln_rows(tok.data_ptr(), wte.data_ptr(), wpe.data_ptr(), V, P, lens.data_ptr(),
                                          h.data_ptr(), C, w.data_ptr(), b.data_ptr(), a.data_ptr(), C, M, C, EPS,
                                          _stream_handle()) == 0
    torch.cuda.synchronize()
    want_h = wte[tok.long()] + wpe[(lens % P).long()]
    assert torch.equal(h[:M], want_h)
    assert _ln_close(a[:M], _ln64(want_h, w, b))
    assert bool((h[M] == 7.0).all()) and bool((a[M] == 7.0).all())
    assert lens.tolist() == lens_l  # read only
    for r in range(M):
        h1, a1 = _embed_one(int(tok[r]), lens_l[r], wte, wpe, w, b, V, P, C)
        assert torch.equal(h[r], h1) and torch.equal(a[r], a1), r


def test_embed_seq_ln_positions_wrap_per_sequence():
    V, P, C, T, B = 1000, 64, 256, 70, 3  # T > n_positions: positions 64 .. 69 wrap to 0 .. 5
    g, wte, wpe, w, b = _embed_tables(V, P, C, seed=22)
    M = B * T
    tok = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
    h = torch.full((M + 1, C), 7.0, device="cuda").half()
    a = torch.full((M + 1, C), 7.0, device="cuda").half()
    f = _lib.lib().ns_lm_embed_seq_ln
    assert f(tok.data_ptr(), wte.data_ptr(), wpe.data_ptr(), V, P, T, h.data_ptr(), C, w.data_ptr(), b.data_ptr(),
             a.data_ptr(), C, M, C, EPS, _stream_handle()) == 0
    torch.cuda.synchronize()
    pos = (torch.arange(M, device="cuda") % T) % P
    want_h = wte[tok.long()] + wpe[pos]
    assert torch.equal(h[:M], want_h)
    assert _ln_close(a[:M], _ln64(want_h, w, b))
    assert bool((h[M] == 7.0).all()) and bool((a[M] == 7.0).all())
    for r in list(range(0, M, 13)) + [T - 1, T, 2 * T - 1, M - 1, P - 1, P, T + P]:
        h1, a1 = _embed_one(int(tok[r]), r % T, wte, wpe, w, b, V, P, C)
        assert torch.equal(h[r], h1) and torch.equal(a[r], a1), r
    assert f(tok.data_ptr(), wte.data_ptr(), wpe.data_ptr(), V, P, T, h.data_ptr(), C, w.data_ptr(), b.data_ptr(),
             a.data_ptr(), C, M - 1, C, EPS, _stream_handle()) == _lib.NS_ERR_CONFIG  # M % T != 0


def test_embed_ln_out_of_range_token_ids_give_nan_rows():
    V, P, C = 1000, 64, 256
    g, wte, wpe, w, b = _embed_tables(V, P, C, seed=23)
    bad = {1: -1, 3: V, 5: 2 ** 31 - 1}
    M = 7
    good = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
    tok = good.clone()
    for r, t in bad.items():
        tok[r] = t
    out = {}
    for name, t in (("good", good), ("bad", tok)):
        h = torch.full((M, C), 7.0, device="cuda").half()
        a = torch.full((M, C), 7.0, device="cuda").half()
        assert _lib.lib().ns_lm_embed_ln(t.data_ptr(), wte.data_ptr(), wpe.data_ptr(), V, P, 9, None, h.data_ptr(), C,
                                         w.data_ptr(), b.data_ptr(), a.data_ptr(), C, M, C, EPS, _stream_handle()) == 0
        out[name] = (h, a)
    torch.cuda.synchronize()
    for r in range(M):
        if r in bad:
            assert bool(torch.isnan(out["bad"][0][r]).all()) and bool(torch.isnan(out["bad"][1][r]).all()), r
        else:  # the neighbours' rows are unaffected
            assert torch.equal(out["bad"][0][r], out["good"][0][r]) and torch.equal(out["bad"][1][r],
                                                                                    out["good"][1][r]), r
    assert torch.equal(out["good"][0], wte[good.long()] + wpe[9])


# ------------------------------------------------------------------------------------------------- layer norms
@pytest.mark.parametrize("M", [1, 9, 1030])
def test_layernorm_rows_advances_every_length_once_per_call(M):
    C = 768
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn((M, C), generator=g, device="cuda").half()
    w = torch.randn((C,), generator=g, device="cuda").half()
    b = torch.randn((C,), generator=g, device="cuda").half()
    y0 = torch.empty((M, C), device="cuda").half()
    y1 = torch.full((M + 1, C), 7.0, device="cuda").half()
    lens0 = torch.randint(0, 5000, (M + 1,), generator=g, device="cuda", dtype=torch.int32)
    lens = lens0.clone()
    L = _lib.lib()
    assert L.ns_lm_layernorm(x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y0.data_ptr(), C, M, C, EPS,
                             _stream_handle()) == 0
    for call in range(1, 4):
        assert L.ns_lm_layernorm_rows(x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y1.data_ptr(), C, M, C, EPS,
                                      lens.data_ptr(), _stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(lens[:M], lens0[:M] + call)
        assert int(lens[M]) == int(lens0[M])  # the guard element past M
    assert torch.equal(y1[:M], y0) and bool((y1[M] == 7.0).all())
    assert _ln_close(y0, _ln64(x, w, b))


@pytest.mark.parametrize("C", [4, 2048])
def test_layernorm_smallest_and_largest_width(C):
    M = 6
    g = torch.Generator(device="cuda").manual_seed(C)
    x = (3 * torch.randn((M, C), generator=g, device="cuda") + 1).half()
    w = torch.randn((C,), generator=g, device="cuda").half()
    b = torch.randn((C,), generator=g, device="cuda").half()
    y = torch.full((M + 1, C), 7.0, device="cuda").half()
    assert _lib.lib().ns_lm_layernorm(x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y.data_ptr(), C, M, C, EPS,
                                      _stream_handle()) == 0
    torch.cuda.synchronize()
    assert _ln_close(y[:M], _ln64(x, w, b))
    assert bool((y[M] == 7.0).all())


@pytest.mark.parametrize("C", [6, 2052])
def test_layernorm_rejects_unsupported_widths(C):
    x = torch.zeros((2, 2056), device="cuda").half()
    w = torch.zeros((2056,), device="cuda").half()
    y = torch.full((2, 2056), 7.0, device="cuda").half()
    L = _lib.lib()
    assert L.ns_lm_layernorm(x.data_ptr(), 2056, w.data_ptr(), w.data_ptr(), y.data_ptr(), 2056, 2, C, EPS,
                             None) == _lib.NS_ERR_UNSUPPORTED
    lens = torch.zeros((2,), dtype=torch.int32, device="cuda")
    assert L.ns_lm_layernorm_rows(x.data_ptr(), 2056, w.data_ptr(), w.data_ptr(), y.data_ptr(), 2056, 2, C, EPS,
                                  lens.data_ptr(), None) == _lib.NS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and lens.tolist() == [0, 0]
