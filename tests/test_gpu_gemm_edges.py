"""GPU: every ns_lm_gemm tile configuration at the edge shapes (csrc/nsg_lm.hip).

test_gpu_lm_kernels.py runs all configurations at N in {768, 1024, 2304} (multiples of every tile width) and K >= 768,
and the ragged / one-K-tile shapes through configuration 6 and the configurations >= 13 only.  Here EVERY configuration
(and the automatic choice), every epilogue, with and without bias, runs at:

* ragged N and M: N no multiple of 64, 128, 192 or 256, down to one 16 x 16 fragment;
* short K: fewer 64-wide K-tiles (1, 2, 3) than LDS pipeline stages (2-4);
* uneven K chains: K/64 tiles that do not divide over the 2 or 4 chains (tiles per chain = ceil(KT / SK): K = 1088 ->
  9 + 8, 1600 -> 13 + 12 (GPT-2-xl's width), 2112 -> 9 + 9 + 9 + 6, 2240 -> 9 + 9 + 9 + 8): gemm_direct, gemm_tiled,
  gemm_persist and gemm_chains each have their own code for the short last chain;
* strided operands (ldx = K + 64, ldw = K + 8, ldy = N + 8): the gap columns of x and wt hold 1000.0, those of y a
  sentinel.

Every configuration returns 0 and gives the SAME BITS as the automatic choice (configurations the host redirects --
persistent with the residual epilogue, the 256 x 256 kernels at K > 1024 -- included: that is the contract); the
automatic choice meets the fp64 bound of test_gemm_matches_fp64_reference, |err| <= 2e-3 |ref| + 2e-3; one guard row
past M and the sentinel columns stay untouched; the residual epilogue reads y from the strided rows.
"""

import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from test_gpu_lm_kernels import EPIS, _operands, _ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 7.0

RAGGED = [(1, 16, 64), (17, 80, 128), (70, 208, 768), (130, 400, 256), (300, 336, 1024)]
SHORT_K = [(200, 320, K) for K in (64, 128, 192)]
UNEVEN_K = [(M, N, K) for K in (1088, 1600, 2112, 2240) for (M, N) in ((5, 64), (70, 256), (300, 384))]
STRIDED = [(70, 208, 768), (300, 384, 1600)]


def _all_configs_agree(M, N, K, epi, strided):
    ldx, ldw, ldy = (K + 64, K + 8, N + 8) if strided else (K, K, N)
    x, wt, bias = _operands(M, N, K, seed=M + 3 * N + 5 * K)
    xs = torch.full((M, ldx), 1000.0, device="cuda").half()
    ws = torch.full((N, ldw), 1000.0, device="cuda").half()
    xs[:, :K], ws[:, :K] = x, wt
    ydt = torch.float32 if epi == "f32" else torch.float16
    y0 = torch.full((M + 1, ldy), SENTINEL, device="cuda").to(ydt)  # one guard row past M, gap columns
    # the residual epilogue adds to what y holds; the others must overwrite every element (NaN until they do)
    y0[:M, :N] = torch.randn((M, N), device="cuda").to(ydt) if epi == "residual" else float("nan")
    L = _lib.lib()
    n = L.ns_lm_gemm_configs()
    assert n >= 20
    for b in (bias, None):
        def run(cfg):
            y = y0.clone()
            rc = L.ns_lm_gemm_config(xs.data_ptr(), ldx, ws.data_ptr(), ldw, b.data_ptr() if b is not None else None,
                                     y.data_ptr(), ldy, M, N, K, EPIS[epi], cfg, _stream_handle())
            assert rc == 0, cfg
            torch.cuda.synchronize()
            return y

        ref = run(-1)
        assert torch.equal(ref[M], y0[M]) and torch.equal(ref[:M, N:], y0[:M, N:])
        want = _ref(x, wt, b, y0[:M, :N], epi)
        err = (ref[:M, :N].double() - want).abs()
        assert bool(torch.isfinite(ref[:M, :N]).all())
        assert bool((err <= 2e-3 * want.abs() + 2e-3).all()), float(err.max())
        # ns_lm_gemm is the automatic choice
        y = y0.clone()
        assert L.ns_lm_gemm(xs.data_ptr(), ldx, ws.data_ptr(), ldw, b.data_ptr() if b is not None else None,
                            y.data_ptr(), ldy, M, N, K, EPIS[epi], _stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
        for cfg in range(n):
            assert torch.equal(run(cfg), ref), (cfg, b is not None)  # the guard row and the gap columns included


@pytest.mark.parametrize("epi", ["store", "gelu", "residual", "f32"])
@pytest.mark.parametrize("M,N,K", RAGGED)
def test_gemm_ragged_n_and_m_every_configuration(M, N, K, epi):
    _all_configs_agree(M, N, K, epi, strided=False)


@pytest.mark.parametrize("epi", ["store", "gelu", "residual", "f32"])
@pytest.mark.parametrize("M,N,K", SHORT_K)
def test_gemm_fewer_k_tiles_than_stages_every_configuration(M, N, K, epi):
    _all_configs_agree(M, N, K, epi, strided=False)


@pytest.mark.parametrize("epi", ["store", "gelu", "residual", "f32"])
@pytest.mark.parametrize("M,N,K", UNEVEN_K)
def test_gemm_uneven_k_chains_every_configuration(M, N, K, epi):
    _all_configs_agree(M, N, K, epi, strided=False)


@pytest.mark.parametrize("epi", ["store", "gelu", "residual", "f32"])
@pytest.mark.parametrize("M,N,K", STRIDED)
def test_gemm_strided_operands_every_configuration(M, N, K, epi):
    _all_configs_agree(M, N, K, epi, strided=True)
