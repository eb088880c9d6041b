"""GPU: the 8-wave 96 x 128 GEMM on a four-deep LDS ring (gemm_ph96, CFG_PH96; csrc/nsg_lm.hip).

Every comparison is bitwise against the two-stage 64 x 64 configuration (CFG_T64_2) through ns_lm_gemm_config on
the same random fp16 operands: all configurations compute every element by the same MFMA chains, so anything but
equality is a staging, wait-count, chain-fold or epilogue fault of the kernel under test.

* K-tile counts around the ring depth (three K-tiles staged ahead, two left in flight by every wait: 1 .. 5 K-tiles
  cover fewer tiles than ring slots) and around the chain boundaries (17 = 9 + 8 and 33 = 9 + 9 + 9 + 6 K-tiles);
* tile edges: M one below, at and one above the 64-row wave-group and 128-row tile edges, N with a 16-wide last
  column tile, one short of and at the 96-column tile, two tiles, and GPT-2's 768;
* the shapes the automatic choice gives this kernel (N = 768, K = 768 and 3072), ragged in M, and the automatic
  choice itself at M = 4096;
* a race screen: the same launch 20 times into fresh buffers, all outputs equal (the inputs are legal and the
  outputs in bounds: it screens the placement of the waits, it provokes nothing);
* guard rows and columns: the output sits inside a larger sentinel-filled buffer that must not change.
"""

import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from test_gpu_lm_kernels import EPIS, _operands  # noqa: E402

pytestmark = pytest.mark.gpu

CFG_T64_2 = 3   # GemmCfg indices (csrc/nsg_lm.hip); existing indices keep their meaning
CFG_PH96 = 24
ALL_EPIS = ["store", "gelu", "residual", "f32"]
SENTINEL = 7.0


def _run(cfg, x, wt, bias, y0, M, N, K, epi, ldy=None, y_off=0):
    """One launch of configuration cfg (None: the automatic choice) into a copy of y0; returns the whole buffer."""
    L = _lib.lib()
    assert L.ns_lm_gemm_configs() > CFG_PH96
    y = y0.clone()
    bp = bias.data_ptr() if bias is not None else None
    yp = y.data_ptr() + y_off * y.element_size()
    ld = ldy if ldy is not None else N
    if cfg is None:
        rc = L.ns_lm_gemm(x.data_ptr(), K, wt.data_ptr(), K, bp, yp, ld, M, N, K, EPIS[epi], _stream_handle())
    else:
        rc = L.ns_lm_gemm_config(x.data_ptr(), K, wt.data_ptr(), K, bp, yp, ld, M, N, K, EPIS[epi], cfg,
                                 _stream_handle())
    assert rc == 0, cfg
    torch.cuda.synchronize()
    return y


def _y0(M, N, epi, seed):
    ydt = torch.float32 if epi == "f32" else torch.float16
    if epi == "residual":  # the residual epilogue adds to what y holds: non-zero
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn((M, N), generator=g, device="cuda").to(ydt)
    return torch.full((M, N), float("nan"), device="cuda").to(ydt)  # must be overwritten everywhere


def _agree(M, N, K, epi, cfgs=(CFG_PH96,), biases=(True, False)):
    x, wt, bias = _operands(M, N, K, seed=M + 3 * N + 5 * K)
    y0 = _y0(M, N, epi, seed=M + N)
    for hb in biases:
        b = bias if hb else None
        ref = _run(CFG_T64_2, x, wt, b, y0, M, N, K, epi)
        assert bool(torch.isfinite(ref).all())
        for cfg in cfgs:
            assert torch.equal(_run(cfg, x, wt, b, y0, M, N, K, epi), ref), (cfg, M, N, K, hb)


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448, 768, 1024, 1088, 2048, 2112, 3072])
def test_tile96_k_tile_counts_around_ring_and_chains(K, epi):
    _agree(200, 208, K, epi)


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 128, 129])
def test_tile96_tile_edges(M, epi):
    for N in (16, 80, 96, 112, 192, 768):
        for K in (192, 1088):
            _agree(M, N, K, epi, biases=(True,))


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("M", [128, 129, 4096 - 37])
def test_tile96_selected_shapes_ragged_residual(M, K):
    _agree(M, 768, K, "residual")


@pytest.mark.parametrize("K", [768, 3072])
def test_tile96_automatic_choice_at_4096(K):
    """ns_lm_gemm itself at the two shapes the automatic choice may hand to this kernel (M >= 4096, N = 768)."""
    _agree(4096, 768, K, "residual", cfgs=(None, CFG_PH96), biases=(True,))


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("K", [768, 3072])
def test_tile96_race_screen(K, epi):
    M, N = 512, 768
    x, wt, bias = _operands(M, N, K, seed=K)
    y0 = _y0(M, N, epi, seed=K + 1)
    ref = _run(CFG_T64_2, x, wt, bias, y0, M, N, K, epi)
    for rep in range(20):
        assert torch.equal(_run(CFG_PH96, x, wt, bias, y0, M, N, K, epi), ref), rep


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("M,N", [(129, 208), (65, 96), (300, 112)])
def test_tile96_guard_rows_and_columns(M, N, epi):
    K, GR, GC = 192, 3, 8  # guard rows above and below, guard columns left and right (16-byte aligned start)
    ldy = N + 2 * GC
    x, wt, bias = _operands(M, N, K, seed=M * N)
    ydt = torch.float32 if epi == "f32" else torch.float16
    y0 = torch.full((M + 2 * GR, ldy), SENTINEL, device="cuda").to(ydt)
    y0[GR:GR + M, GC:GC + N] = _y0(M, N, epi, seed=M)
    off = GR * ldy + GC
    ref = _run(CFG_T64_2, x, wt, bias, y0, M, N, K, epi, ldy=ldy, y_off=off)
    outside = torch.ones_like(y0, dtype=torch.bool)
    outside[GR:GR + M, GC:GC + N] = False
    y = _run(CFG_PH96, x, wt, bias, y0, M, N, K, epi, ldy=ldy, y_off=off)
    assert torch.equal(y[outside], y0[outside])  # bitwise: the sentinel is exact in both formats
    assert torch.equal(y, ref)
