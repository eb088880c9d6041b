"""CPU: the fp64 reference of ``tests/lm_reference.py`` is GPT-2, ``gather_kv`` reads pages right, and the constants
of ``tests/test_gpu_lm_truth.py`` make that test able to tell a wrong kernel from a right one.

* ``reference_forward`` equals ``GPT2LMHeadModel.double()`` (weights rounded to fp16 first, wrapped
  ``position_ids``) within 1e-9, logits and ``past_key_values``, over more than two wraps; ``window=W`` equals the same
  model under the band mask.
* ``gather_kv`` returns hand-filled rows, scattered over two pool segments, in position order (fp16 and fp8 pages).
* For every model, seed and token stream of the GPU test (``lm_reference.CASES``), from the reference alone and with
  the largest margin a case may ever take (``M_MAX``): (a) positions one off from the first wrapped row on move EVERY
  later logits row by at least 20 x the logit tolerance; (b) K rows and V rows at adjacent positions differ by at
  least 20 x the fp16 row tolerance in every layer; (c) no stream holds id ``vocab - 1`` and the streams' tokens
  differ at every step.  For the fp8 pages of case E the row tolerance carries half an e4m3fn step per element
  (about |x| / 16), so the condition is stated per element: a stored row put at an adjacent position exceeds the
  elementwise tolerance at some element by a factor of 20 at least.
"""

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_reference as R
from neuralsteganography_amd.lm.kvpages import KVPagePool, PagedKV

# e16 (Hugging Face's fp16 forward against the fp64 reference) is computed where tests/test_gpu_lm_truth.py computes it
# when there is a GPU, by PyTorch's own kernels: some CPUs take seconds per sequence for the 768-wide model's fp16
# products.  Nothing of the library runs here either way.
E16_DEVICE = "cuda" if torch.cuda.is_available() else "cpu"


@pytest.fixture(scope="module")
def hf_double():
    model = R.model_of("M0")
    return model, copy.deepcopy(model).half().double().eval()


def _hf(md, ids, mask=None):
    T = len(ids)
    pos = (torch.arange(T) % md.config.n_positions)[None]
    with torch.no_grad():
        out = md(input_ids=torch.as_tensor(ids)[None], position_ids=pos, attention_mask=mask, use_cache=True)
    K, V = R.past_kv(out.past_key_values)
    return out.logits[0], K, V


def test_reference_equals_hugging_face_in_float64(hf_double):
    model, md = hf_double
    ids = np.random.default_rng(5).integers(0, R.VOCAB, size=150)  # more than two wraps of the 64 positions
    ref = R.reference_forward(model.state_dict(), ids, model.config.n_head)
    lg, K, V = _hf(md, ids)
    assert ref.logits.shape == (150, R.VOCAB) and len(ref.K) == 2 and ref.K[0].shape == (2, 150, 64)
    assert float((lg - ref.logits).abs().max()) < 1e-9
    for a, b in zip(K + V, ref.K + ref.V):
        assert float((a - b).abs().max()) < 1e-9
    # the wrap is in the comparison: unwrapped positions would not even index the table, and shifted ones differ
    wrong = R.reference_forward(model.state_dict(), ids, 2, positions=R.off_by_one_positions(150, 64))
    assert float((wrong.logits[:64] - ref.logits[:64]).abs().max()) == 0.0
    assert float((wrong.logits[64:] - ref.logits[64:]).abs().amax(1).min()) > 0.1


@pytest.mark.parametrize("W", [1, 48, 64])
def test_window_equals_hugging_face_under_the_band_mask(hf_double, W):
    model, md = hf_double
    ids = np.random.default_rng(6).integers(0, R.VOCAB, size=150)
    t = torch.arange(150)
    band = (t[None, :] <= t[:, None]) & (t[None, :] > t[:, None] - W)
    lg, K, V = _hf(md, ids, mask=band[None, None])
    ref = R.reference_forward(model.state_dict(), ids, 2, window=W)
    assert float((lg - ref.logits).abs().max()) < 1e-9
    for a, b in zip(K + V, ref.K + ref.V):
        assert float((a - b).abs().max()) < 1e-9
    full = R.reference_forward(model.state_dict(), ids, 2)
    assert float((full.logits[:W] - ref.logits[:W]).abs().max()) < 1e-12  # the window has not cut anything yet
    assert float((full.logits[W + 1:] - ref.logits[W + 1:]).abs().amax(1).min()) > 1e-6
    # rows of a context (exact_below) are never windowed: the native prefill is plain causal attention
    mixed = R.reference_forward(model.state_dict(), ids, 2, window=W, exact_below=100)
    assert float((mixed.K[1][:, :100] - full.K[1][:, :100]).abs().max()) == 0.0


def test_fp8_option_quantises_the_own_row_and_spares_the_context_queries():
    model = R.model_of("M0")
    ids = np.random.default_rng(8).integers(0, R.VOCAB, size=90)
    sd = model.state_dict()
    full = R.reference_forward(sd, ids, 2)
    q = R.reference_forward(sd, ids, 2, kv="fp8")
    for a, x in zip(q.K + q.V, q.K_exact + q.V_exact):
        assert torch.equal(a, R.fp8_round(x)) and torch.equal(a, a.to(torch.float8_e4m3fn).double())
    assert torch.equal(q.K_exact[0], full.K[0])  # layer 0's K/V do not depend on the attention at all
    # row 0 attends only itself: its layer-1 K differs from the fp16-KV one only because its own V was quantised
    assert float((q.K_exact[1][:, 0] - full.K[1][:, 0]).abs().max()) > 0.0
    mixed = R.reference_forward(sd, ids, 2, kv="fp8", exact_below=40)
    assert torch.equal(mixed.K_exact[1][:, :40], full.K[1][:, :40])
    assert torch.equal(mixed.logits[:40], full.logits[:40])
    assert float((mixed.logits[40:] - full.logits[40:]).abs().amax(1).min()) > 0.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.uint8])
def test_gather_kv_reads_hand_filled_pages_in_order(dtype):
    H, D, n_layer, T0 = 2, 64, 3, 5
    pool = KVPagePool(n_layer=n_layer, n_head=H, head_dim=D, dtype=dtype, device="cpu", seg_pages=2)
    kv = PagedKV(pool, 2, T0, 1)
    for upto in (T0 + 20, T0 + 40, T0 + 70):  # the two slots take pages in turn: each slot's are scattered
        for s in (1, 0):
            assert kv.ensure([s], [upto - 7 * s]).size == 0
    kv.set_lens([0, 1], [T0 + 70, T0 + 33])
    assert len(pool.segments) >= 2
    g = torch.Generator().manual_seed(3)

    def rand(*shape):
        x = torch.randn(shape, generator=g).half()
        return x if dtype == torch.float16 else x.to(torch.float8_e4m3fn).view(torch.uint8)

    def widen(x):
        return (x.view(torch.float8_e4m3fn) if x.dtype == torch.uint8 else x).double()

    for seg in pool.segments:
        seg.copy_(rand(*seg.shape))  # whatever a page holds beyond the rows written below must not come back
    kp, vp = rand(n_layer, 1, H, T0, D), rand(n_layer, 1, H, T0, D)
    want = {}
    segs_used = set()
    for s, L in ((0, T0 + 70), (1, T0 + 33)):
        for layer in range(n_layer):
            k, v = rand(H, L - T0, D), rand(H, L - T0, D)
            for r in range(L - T0):  # by hand: address -> (segment, page), then [layer][page][K|V][H][32][D]
                addr = int(kv.host[s, r // 32])
                (si, pg), = [(i, (addr - sg.data_ptr()) // pool.block_bytes) for i, sg in enumerate(pool.segments)
                             if 0 <= addr - sg.data_ptr() < pool.seg_pages * pool.block_bytes]
                segs_used.add((s, si))
                blk = pool.segments[si][layer, pg].view(2, H, 32, D)
                blk[0, :, r % 32] = k[:, r]
                blk[1, :, r % 32] = v[:, r]
            want[s, layer] = (torch.cat([widen(kp[layer, 0]), widen(k)], 1), torch.cat([widen(vp[layer, 0]), widen(v)], 1))
    assert len({si for s, si in segs_used if s == 0}) >= 2  # slot 0's rows really lie in two segments
    lm = SimpleNamespace(kv=kv, kp=kp, vp=vp)
    before = [seg.clone() for seg in pool.segments]
    table0, free0 = kv.host.copy(), pool.free_pages
    for (s, layer), (k, v) in want.items():
        gk, gv = R.gather_kv(lm, s, layer)
        assert gk.dtype == torch.float64 and gk.shape == k.shape
        assert torch.equal(gk, k) and torch.equal(gv, v), (s, layer)
    assert all(torch.equal(a, b) for a, b in zip(before, pool.segments))  # read only
    assert np.array_equal(table0, kv.host) and pool.free_pages == free0
    kv.set_lens([1], [T0 - 0])  # a slot at the shared context alone: only the prefix rows
    gk, _ = R.gather_kv(lm, 1, 0)
    assert torch.equal(gk, widen(kp[0, 0]))
    kv.table[0, 1] += 2  # an address that is no page of the pool is an error, not a silent read
    with pytest.raises(AssertionError):
        R.gather_kv(lm, 0, 0)


def _refs(name, **opts):
    c = R.CASES[name]
    model = R.model_of(c["model"])
    seqs = R.case_sequences(name)
    ctx_len = [len(x) for x in R.case_streams(name)[0]]
    sd, H = model.state_dict(), model.config.n_head
    plain = [R.reference_forward(sd, s, H) for s in seqs]
    e16 = R.e16_of(model, seqs, plain, device=E16_DEVICE)
    if opts:
        refs = [R.reference_forward(sd, s, H, exact_below=n, **opts) for s, n in zip(seqs, ctx_len)]
    else:
        refs = plain
    e8 = max(float((r.logits - p.logits).abs().max()) for r, p in zip(refs, plain)) if opts.get("kv") == "fp8" else 0.0
    return c, model, seqs, refs, e16, e8


CONDITION_RUNS = [(n, {}) for n in R.CASES if n != "E"] + [("E", {"kv": "fp8"}), ("E", {"window": R.E_WINDOW})]


@pytest.mark.parametrize("name,opts", CONDITION_RUNS, ids=[n + "".join("-" + str(v) for v in o.values())
                                                            for n, o in CONDITION_RUNS])
def test_conditions_that_make_the_gpu_test_meaningful(name, opts):
    c, model, seqs, refs, (e_l, e_r), e8 = _refs(name, **opts)
    n_pos, V = model.config.n_positions, model.config.vocab_size
    assert c["m"] in (1, 2, 4, 8) and c["m"] <= R.M_MAX
    sd, H = model.state_dict(), model.config.n_head
    ctx_len = [len(x) for x in R.case_streams(name)[0]]
    amax = max(float(r.logits.abs().max()) for r in refs)
    ltol = R.logit_tol(R.M_MAX, e_l, c["logits"], amax) + 0.5 * e8  # e8: the fp8 allowance of the GPU test
    rtol = R.row_tol(R.M_MAX, e_r)
    worst_a = worst_b = worst_b8 = float("inf")
    for s, r, n in zip(seqs, refs, ctx_len):
        assert len(s) > n_pos  # every stream wraps
        wrong = R.reference_forward(sd, s, H, positions=R.off_by_one_positions(len(s), n_pos), exact_below=n, **opts)
        d = (wrong.logits - r.logits).abs().amax(1)
        assert float(d[:n_pos].max()) == 0.0
        worst_a = min(worst_a, float(d[n_pos:].min()))
        for rows, exact in zip(r.K + r.V, r.K_exact + r.V_exact):
            worst_b = min(worst_b, float((exact[:, 1:] - exact[:, :-1]).abs().amax((0, 2)).min()))
            if opts.get("kv") == "fp8":  # the stored (quantised) neighbour against the elementwise fp8 tolerance
                tol = R.row_tol(R.M_MAX, e_r, exact)
                worst_b8 = min(worst_b8, float(((rows[:, 1:] - exact[:, :-1]).abs() / tol[:, :-1]).amax((0, 2)).min()),
                               float(((rows[:, :-1] - exact[:, 1:]).abs() / tol[:, 1:]).amax((0, 2)).min()))
    print(f"{name} {opts}: e16 logits {e_l:.3g} rows {e_r:.3g}; (a) {worst_a:.3g} vs 20 x {ltol:.3g}; "
          f"(b) {worst_b:.3g} vs 20 x {rtol:.3g}; e8 {e8:.3g}; fp8 swap factor {worst_b8:.3g}")
    assert worst_a >= 20 * ltol  # (a)
    assert worst_b >= 20 * rtol  # (b)
    if opts.get("kv") == "fp8":
        assert worst_b8 >= 20.0
    contexts, steps = R.case_streams(name)  # (c)
    assert max(max(x) for x in seqs) < V - 1 and min(min(x) for x in seqs) >= 0
    assert steps.shape == (c["steps"], c["B"]) and len(contexts) == c["B"]
    assert all(len(set(row.tolist())) == c["B"] for row in steps)


def test_case_d_contexts_are_the_issue_s():
    contexts, _ = R.case_streams("D")
    assert [len(x) for x in contexts] == [1, 31, 32, 33, 64, 65, 100, 200, 100, 33]
    assert contexts[8] == contexts[6] and contexts[9] == contexts[3]
    assert len({tuple(x) for x in contexts}) == 8
    assert sorted(R.D_SLOT_ORDER) == list(range(10)) and R.D_SLOT_ORDER != list(range(10))
