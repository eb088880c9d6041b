"""GPU: ns_lm_head_score (include/nsg_score.h) -- the head GEMM with the row scores as its epilogue -- and the
scorer's two switches, ``packed`` and ``fused_head``.

1. The kernel against float64: ``want`` is the float64 log-softmax of the logits ``ns_lm_gemm`` itself stores for the
   same operands (the kernel's logits are those bits by construction), compared as ``ns_score_rows`` is compared in
   test_gpu_guard.py: ``|got - want| / (|want| + 1) < 2e-5``, the project's tolerance for fp32 partial sums (DESIGN
   §4b).  V not a multiple of the 128-column tile (61: less than one tile), M not a multiple of the 128-row tile,
   labels -1 / 0 / V-1 / >= V, a flat row, a row with one dominant column, rows past M untouched.
2. Batch invariance: a row's two outputs have the same bits alone (M = 1) and inside M = 130 and M = 1030.
3. The host's argument checks.
4. ``HipLMScorer(packed=True)`` gives the floats of ``packed=False`` for every text.
5. ``fused_head=True`` against the default path, alone against inside a batch, and against the Hugging Face formulas.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5  # fp32 partials, merged in float64


def _operands(M, V, K, seed):
    """x [M, K] and wt [V rounded up to 16, K] fp16 (zero rows past V: ns_lm_gemm needs N % 16 == 0).  Row 3 of x is
    zero (flat logits); weight row 5 is doubled and row 4 of x points along it (one dominant column)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    vp = (V + 15) // 16 * 16
    wt = torch.zeros((vp, K), device="cuda", dtype=torch.float16)
    wt[:V] = (torch.randn((V, K), generator=g, device="cuda") * 0.06).half()
    x = torch.randn((M, K), generator=g, device="cuda").half()
    wt[5] *= 2.0
    if M > 4:
        x[3] = 0.0
        x[4] = torch.sign(wt[5]) * 4.0  # logit 5 of row 4: about 0.4 K, the others a few units
    return x, wt


def _labels(M, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    lab = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
    for i, v in enumerate((V - 1, -1, 0, V, 5, V + 7)):  # row 4 (dominant column 5) is labelled with it
        if i < M:
            lab[i] = v
    return lab


def _gemm_logits(x, wt, V, dtype):
    """The logits ns_lm_gemm stores: fp32 (STORE_F32) or fp16 (STORE)."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _stream_handle

    M, K = x.shape
    y = torch.empty((M, wt.shape[0]), device="cuda", dtype=torch.float16 if dtype == "f16" else torch.float32)
    epi = _lib.NS_LM_EPI_STORE if dtype == "f16" else _lib.NS_LM_EPI_STORE_F32
    rc = _lib.lib().ns_lm_gemm(x.data_ptr(), x.stride(0), wt.data_ptr(), wt.stride(0), None, y.data_ptr(),
                               y.stride(0), M, wt.shape[0], K, epi, _stream_handle())
    assert rc == 0
    return y[:, :V]


def _head_score(x, wt, V, dtype, lab, M=None, pad=2):
    """ns_lm_head_score over the first ``M`` rows of x: (rc, nll, ent), outputs ``M + pad`` long and NaN-filled."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _stream_handle

    L = _lib.lib()
    M = x.shape[0] if M is None else M
    K = x.shape[1]
    nll = torch.full((M + pad,), float("nan"), dtype=torch.float64, device="cuda")
    ent = torch.full_like(nll, float("nan"))
    nbytes = int(L.ns_lm_head_score_work_bytes(M, V))
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = L.ns_lm_head_score(x.data_ptr(), x.stride(0), wt.data_ptr(), wt.stride(0), M, V, K,
                            _lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32, lab.data_ptr(),
                            nll.data_ptr(), ent.data_ptr(), work.data_ptr(), nbytes, _stream_handle())
    torch.cuda.synchronize()
    return rc, nll, ent


@pytest.mark.parametrize("M,V,K,dtype", [(37, 50257, 768, "f32"), (37, 50257, 768, "f16"), (130, 700, 128, "f32"),
                                         (5, 61, 128, "f16"), (1, 2000, 128, "f32")])
def test_head_score_matches_float64_reference(M, V, K, dtype):
    x, wt = _operands(M, V, K, seed=V + M)
    lab = _labels(M, V, seed=V)
    rc, nll, ent = _head_score(x, wt, V, dtype, lab)
    assert rc == 0
    lp = torch.log_softmax(_gemm_logits(x, wt, V, dtype).double(), -1)
    valid = (lab >= 0) & (lab < V)
    want_nll = torch.where(valid, -lp.gather(1, lab.clamp(0, V - 1).long()[:, None])[:, 0], torch.zeros_like(lp[:, 0]))
    want_ent = -(lp.exp() * lp).sum(-1)
    if M > 4:
        assert want_ent[3].item() == pytest.approx(np.log(V), rel=1e-9)  # the flat row
        assert want_ent[4].item() < 1e-3 and lab[4].item() == 5  # the dominant column, labelled
    for name, got, want in (("nll", nll, want_nll), ("ent", ent, want_ent)):
        assert torch.isfinite(got[:M]).all(), name
        assert torch.isnan(got[M:]).all(), name  # rows past M are not written
        err = (got[:M] - want).abs() / (want.abs() + 1.0)
        print(f"{name} M={M} V={V} K={K} {dtype}: max err {err.max().item():.3e}")
        assert err.max().item() < TOL, (name, err.max().item())
    assert (nll[:M][~valid] == 0.0).all()  # no label, or one outside [0, V)


@pytest.fixture(scope="module")
def wide():
    """1,030 rows against GPT-2's vocabulary, made once."""
    M, V, K = 1030, 50257, 768
    x, wt = _operands(M, V, K, seed=99)
    return x, wt, V, _labels(M, V, seed=98)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_head_score_is_batch_invariant(wide, dtype):
    x, wt, V, lab = wide
    runs = {}
    for M in (130, 1030):
        rc, nll, ent = _head_score(x, wt, V, dtype, lab, M=M)
        assert rc == 0
        runs[M] = (nll, ent)
    for r in (0, 4, 77, 129, 1029):
        rc, nll, ent = _head_score(x[r:r + 1].clone(), wt, V, dtype, lab[r:r + 1].clone())
        assert rc == 0
        for M in (130, 1030):
            if r < M:
                assert nll[0].item() == runs[M][0][r].item(), (r, M)
                assert ent[0].item() == runs[M][1][r].item(), (r, M)
    assert torch.equal(runs[130][0][:130], runs[1030][0][:130]) and torch.equal(runs[130][1][:130], runs[1030][1][:130])


def test_head_score_argument_checks():
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _stream_handle

    L = _lib.lib()
    M, V, K = 8, 300, 128
    x, wt = _operands(M, V, K, seed=1)
    lab = _labels(M, V, seed=1)
    nll = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    ent = torch.full_like(nll, float("nan"))
    nbytes = int(L.ns_lm_head_score_work_bytes(M, V))
    assert nbytes == 1 * M * 16 + M * 4  # 300 columns: 3 tiles, one span
    assert int(L.ns_lm_head_score_work_bytes(M, 50257)) == 99 * M * 16 + M * 4  # 393 tiles in spans of 4
    assert int(L.ns_lm_head_score_work_bytes(0, V)) == 0
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _stream_handle()

    def call(xp=x.data_ptr(), ldx=K, wp=wt.data_ptr(), m=M, k=K, np_=nll.data_ptr(), ep=ent.data_ptr(),
             wk=work.data_ptr(), wb=nbytes, dt=_lib.NS_DTYPE_F32):
        return L.ns_lm_head_score(xp, ldx, wp, K if k == K else k, m, V, k, dt, lab.data_ptr(), np_, ep, wk, wb, st)

    assert call(xp=None) == _lib.NS_ERR_CONFIG
    assert call(wp=None) == _lib.NS_ERR_CONFIG
    assert call(wk=None) == _lib.NS_ERR_CONFIG
    assert call(wb=nbytes - 1) == _lib.NS_ERR_CONFIG
    assert call(ldx=K + 4) == _lib.NS_ERR_CONFIG  # rows no longer 16-byte aligned
    assert call(xp=x.data_ptr() + 2) == _lib.NS_ERR_CONFIG
    assert call(dt=_lib.NS_DTYPE_F64) == _lib.NS_ERR_CONFIG
    assert call(m=0) == _lib.NS_OK
    assert call(np_=None, ep=None) == _lib.NS_OK
    torch.cuda.synchronize()
    assert torch.isnan(nll).all() and torch.isnan(ent).all()  # none of the calls above launched
    # K of more than one accumulator chain: refused before any launch (the operands here are only K = 128 wide)
    assert call(k=2048, ldx=2048) == _lib.NS_ERR_UNSUPPORTED
    assert call(k=96, ldx=96) == _lib.NS_ERR_UNSUPPORTED  # no multiple of the 64-wide K tile
    torch.cuda.synchronize()
    assert torch.isnan(nll).all()
    assert call(ep=None) == _lib.NS_OK  # one output alone
    torch.cuda.synchronize()
    assert torch.isfinite(nll).all() and torch.isnan(ent).all()


# ------------------------------------------------------------------------------------------------------ scorer
TEXT_LENS = (1, 2, 63, 64, 65, 130)


def _texts():
    rng = np.random.default_rng(7)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    return ["".join(rng.choice(letters, size=n)) for n in TEXT_LENS] + ["", "  "]


@pytest.fixture(scope="module")
def tiny_native():
    """fp16 native GPT-2 (2 layers, 2 heads of 64, vocabulary 2,000) with the byte tokenizer, and its fp32 parent."""
    from neuralsteganography_amd.lm.arithmetic import ByteTokenizer
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2

    m = random_gpt2("tiny", vocab_size=2000, n_positions=256, n_embd=128, n_head=2, seed=31)
    lm = BatchedGPT2(m, device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    assert lm.native
    return m, lm, ByteTokenizer(2000)


def _same(a, b):
    return a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("rows_per_batch", [96, 32768])
def test_packed_scorer_equals_padded(tiny_native, rows_per_batch):
    from neuralsteganography_amd.metrics import HipLMScorer

    _, lm, tok = tiny_native
    texts = _texts()
    packed = HipLMScorer(lm, tok, rows_per_batch=rows_per_batch)
    padded = HipLMScorer(lm, tok, rows_per_batch=rows_per_batch, packed=False)
    assert packed.packed and not packed.fused_head and not padded.packed  # the defaults for a native model
    got, want = packed.metrics_batch(texts), padded.metrics_batch(texts)
    for t, g, w in zip(texts, got, want):
        assert set(g) == set(w) and all(_same(g[k], w[k]) for k in g), (len(t), g, w)
    real = sum(TEXT_LENS)
    assert packed.last_rows["rows"] == packed.last_rows["real"] == real  # no padding row computed
    assert padded.last_rows["real"] == real and padded.last_rows["rows"] > real
    if rows_per_batch == 96:
        assert packed.last_rows["groups"] > 1 and padded.last_rows["groups"] > 1
    else:
        assert packed.last_rows["groups"] == 1


def test_fused_scorer(tiny_native):
    from test_gpu_guard import _hf_metrics

    from neuralsteganography_amd.metrics import HipLMScorer

    m, lm, tok = tiny_native
    texts = _texts()
    base = HipLMScorer(lm, tok).metrics_batch(texts)
    fused = HipLMScorer(lm, tok, fused_head=True)
    got = fused.metrics_batch(texts)
    for t, g, w in zip(texts, got, base):
        assert g["token_count"] == w["token_count"]
        for k in ("avg_nll", "avg_entropy"):
            if isinstance(w[k], float) and np.isnan(w[k]):
                assert np.isnan(g[k])
                continue
            print(f"len {len(t)} {k}: fused {g[k]!r} default {w[k]!r}")
            assert abs(g[k] - w[k]) <= 4e-5 * (abs(w[k]) + 1.0), (len(t), k, g[k], w[k])
    # alone and among 64 others: identical floats
    rng = np.random.default_rng(11)
    others = ["".join(rng.choice(list("abcdefgh "), size=int(rng.integers(2, 200)))).strip() or "x" for _ in range(64)]
    crowd = fused.metrics_batch(others[:30] + texts + others[30:])
    small = HipLMScorer(lm, tok, fused_head=True, rows_per_batch=96).metrics_batch(texts)
    for i, g in enumerate(got):
        assert all(_same(g[k], crowd[30 + i][k]) for k in g), i
        assert all(_same(g[k], small[i][k]) for k in g), i
    # the Hugging Face formulas, at the fp16 tolerance of test_hip_lm_scorer_matches_hf_formulas
    tol = 3e-2
    for t, g in zip(texts, got):
        ids = tok.encode(t)
        if len(ids) < 2 or not t.split():
            continue
        nll, ent = _hf_metrics(m, ids)
        assert abs(g["avg_nll"] - nll) < tol and abs(g["avg_entropy"] - ent) < tol
        assert abs(g["ppl"] - np.exp(nll)) < tol * np.exp(nll) * 2


def test_fused_scorer_falls_back_on_wide_models():
    """A width of more than one accumulator chain (C = 1088 > 1024): ns_lm_head_score refuses it and the scorer runs
    the two launches -- the default path's floats exactly."""
    from neuralsteganography_amd.lm.arithmetic import ByteTokenizer
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2
    from neuralsteganography_amd.metrics import HipLMScorer

    m = random_gpt2("tiny", vocab_size=300, n_positions=64, n_embd=1088, n_head=17, n_layer=1, seed=5)
    lm = BatchedGPT2(m, device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float32)
    tok = ByteTokenizer(300)
    texts = ["a wide model", "xy"]
    assert HipLMScorer(lm, tok, fused_head=True).metrics_batch(texts) == HipLMScorer(lm, tok).metrics_batch(texts)


def test_scorer_switches_are_validated():
    from neuralsteganography_amd.lm.arithmetic import ByteTokenizer
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2
    from neuralsteganography_amd.metrics import HipLMScorer

    m = random_gpt2("tiny", vocab_size=300, n_positions=64, seed=5)
    lm = BatchedGPT2(m, device="cuda", compute_dtype=torch.float32, logits_dtype=torch.float32)
    assert not HipLMScorer(lm, ByteTokenizer(300)).packed  # a non-native model keeps the padded path
    with pytest.raises(ValueError):
        HipLMScorer(lm, ByteTokenizer(300), packed=True)
    with pytest.raises(ValueError):
        HipLMScorer(lm, ByteTokenizer(300), fused_head=True)
