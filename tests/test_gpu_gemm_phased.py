"""GPU: the phase-pipelined GEMM (gemm_ph) and the 96 x 128 tiles of gemm_tiled (csrc/nsg_lm.hip).

Every comparison is bitwise against the two-stage 64 x 64 configuration (CFG_T64_2) on the same random fp16
operands: all configurations compute every element by the same MFMA chain, so anything but equality is a staging,
wait-count or epilogue fault of the configuration under test.

* K-tile counts around the pipeline: gemm_ph issues a K-tile's copies up to two K-tiles ahead and leaves up to
  four units in flight, so 1 .. 16 K-tiles cover fewer tiles than units in flight, odd and even counts;
* tile edges: M and N one below, at and one above the 128 / 256 row and 96 / 192 / 256 column tile edges;
* the one-tile-per-CU shapes of the 96 x 128 tiles (N = 768), ragged in M, one K chain and four (K = 3072);
* a race screen: the same launch 20 times into fresh buffers, all outputs equal (the inputs are legal and the
  outputs in bounds: it screens the placement of the waits, it provokes nothing);
* guard rows and columns: the output sits inside a larger sentinel-filled buffer that must not change.

gemm_ph runs one tile per workgroup (the persistent form measured no faster and was not kept), so there is no
grid-relative case.
"""

import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from test_gpu_lm_kernels import EPIS, _operands  # noqa: E402

pytestmark = pytest.mark.gpu

CFG_T64_2 = 3                      # GemmCfg indices (csrc/nsg_lm.hip); existing indices keep their meaning
CFG_T96x128_3, CFG_T96x128_4, CFG_PH256, CFG_PH192 = 20, 21, 22, 23
NEW = (CFG_T96x128_3, CFG_T96x128_4, CFG_PH256, CFG_PH192)
ALL_EPIS = ["store", "gelu", "residual", "f32"]
SENTINEL = 7.0


def _run(cfg, x, wt, bias, y0, M, N, K, epi, ldy=None, y_off=0):
    """One launch of configuration cfg into a copy of y0; returns the whole buffer."""
    L = _lib.lib()
    assert L.ns_lm_gemm_configs() > max(NEW)
    y = y0.clone()
    rc = L.ns_lm_gemm_config(x.data_ptr(), K, wt.data_ptr(), K, bias.data_ptr() if bias is not None else None,
                             y.data_ptr() + y_off * y.element_size(), ldy if ldy is not None else N, M, N, K,
                             EPIS[epi], cfg, _stream_handle())
    assert rc == 0, cfg
    torch.cuda.synchronize()
    return y


def _y0(M, N, epi, seed):
    ydt = torch.float32 if epi == "f32" else torch.float16
    if epi == "residual":  # the residual epilogue adds to what y holds: non-zero
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn((M, N), generator=g, device="cuda").to(ydt)
    return torch.full((M, N), float("nan"), device="cuda").to(ydt)  # must be overwritten everywhere


def _agree(M, N, K, epi, cfgs=NEW, biases=(True, False)):
    x, wt, bias = _operands(M, N, K, seed=M + 3 * N + 5 * K)
    y0 = _y0(M, N, epi, seed=M + N)
    for hb in biases:
        b = bias if hb else None
        ref = _run(CFG_T64_2, x, wt, b, y0, M, N, K, epi)
        assert bool(torch.isfinite(ref).all())
        for cfg in cfgs:
            assert torch.equal(_run(cfg, x, wt, b, y0, M, N, K, epi), ref), (cfg, M, N, K, hb)


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448, 768, 1024])
def test_phased_k_tile_counts_around_the_pipeline(K, epi):
    _agree(300, 400, K, epi)


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("M", [1, 127, 128, 129, 255, 256, 257])
def test_phased_tile_edges(M, epi):
    for N in (16, 96, 176, 192, 208, 256, 272, 768):
        _agree(M, N, 192, epi, biases=(True,))


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("M", [128, 129, 4096 - 37])
def test_one_tile_per_cu_shapes_residual(M, K):
    """N = 768: 8 column tiles of 96; K = 3072 runs gemm_tiled's SPLIT form (four chains) -- the 256 x 256
    configurations are redirected there by the host, same bits."""
    _agree(M, 768, K, "residual")


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("M,N,K", [(512, 4112, 768), (512, 3072, 768)])
def test_phased_race_screen(M, N, K, epi):
    x, wt, bias = _operands(M, N, K, seed=N)
    y0 = _y0(M, N, epi, seed=N + 1)
    ref = _run(CFG_T64_2, x, wt, bias, y0, M, N, K, epi)
    for cfg in NEW:
        for rep in range(20):
            assert torch.equal(_run(cfg, x, wt, bias, y0, M, N, K, epi), ref), (cfg, rep)


@pytest.mark.parametrize("epi", ALL_EPIS)
@pytest.mark.parametrize("M,N", [(129, 208), (257, 400), (300, 96)])
def test_phased_guard_rows_and_columns(M, N, epi):
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
    for cfg in NEW:
        y = _run(cfg, x, wt, bias, y0, M, N, K, epi, ldy=ldy, y_off=off)
        assert torch.equal(y[outside], y0[outside]), cfg  # bitwise: the sentinel is exact in both formats
        assert torch.equal(y, ref), cfg
