"""GPU: every fp16 pattern and every e4m3 byte through the fp8 KV cache's conversion sites (csrc/nsg_attn.hip).

The other fp8 tests draw K and V from N(0, 1): a narrow band of exponents, nothing near the +-448 saturation edge, no
non-finite value.  Here (inputs and expected values from tests/fp8_cases.py, whose soundness
tests/test_fp8_cases_host.py checks on the CPU):

(a) ``ns_quantize_fp8`` on all 65,536 fp16 patterns, at each position of a packed word: bit-equal to the from-spec
    integer reference; a NaN gives a NaN byte.
(b) the same patterns as the new token's k and v through every append site -- the lockstep kernel, the paged kernel
    (short path, general path, one pair per workgroup), the chunk kernel (C = 1, 4) and the page store of the ragged
    prefill: the stored bytes equal the quantiser's, no other byte of the cache or pool changes.
(c) the V dequantiser (``FmtF8::unpack``): every byte at every head dim with softmax weight exactly 1: the output
    element is deq(byte), exactly; a NaN byte gives NaN in that element only.
(d) the K dequantiser (``FmtF8::dot``): every byte at every head dim as the only non-zero of a key row:
    output[0] = sigmoid(c deq(byte)) within 2^-10 (derived in fp8_cases.K_TOL); a NaN byte gives NaN.
(e) attention with outlier dimensions (K and V scaled per head dim by 24 and 200) against float64, the tolerance of
    tests/test_gpu_attention_probes.py unchanged.
(f) the same-bits contracts (paged == lockstep, chunk == one token per call) on caches of uniformly random non-NaN
    bytes: magnitudes log-uniform up to 448.
(g) a stream whose k/v row was NaN once stays NaN: its next step's output is NaN with an fp8 cache as with an fp16
    one, and no other stream's output or cache byte differs from a run where that stream was finite.

NaN values are data here: every launch is a legal one.
"""

import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fp8_cases as fc  # noqa: E402
import test_gpu_attention_chunk as chunk_tests  # noqa: E402
from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import ragged_blocks  # noqa: E402
from test_gpu_attention_probes import (_launch, _paged_lengths, attention_ref, build_case, to_fp8,  # noqa: E402
                                       tolerance)

pytestmark = pytest.mark.gpu

D = 64
SCALE = D ** -0.5
LAYER, NLAYER = 1, 2  # the pages hold two layers; the kernels work on the second


# ------------------------------------------------------------------------------------------------------ plumbing
def _q8(t):
    out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    assert _lib.lib().ns_quantize_fp8(t.contiguous().data_ptr(), out.data_ptr(), t.numel(), _stream_handle()) == 0
    return out


def _same(a, b):
    """Bit equality (NaN patterns included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _rand_cache(shape, g, fp8):
    """Cache filler: uniformly random non-NaN bytes, or N(0, 1) fp16."""
    return fc.random_finite_bytes(shape, g, "cuda") if fp8 else torch.randn(shape, generator=g, device="cuda").half()


def _state(B, H, T0, lens, qkv, dk, dv, kp=None, vp=None, fp8=True):
    """One decode step's inputs: qkv [B (* C), 3 H D] fp16; the streams' own rows dk / dv [B, H, rows, D] (row r =
    position T0 + r, rows a multiple of 32); the shared prefix kp / vp [H, T0, D]; lens [B] cached positions."""
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (B,)).copy()
    rows = dk.shape[2]
    assert rows % 32 == 0 and int(lens.min()) >= T0 and dk.shape == dv.shape == (B, H, rows, D)
    if kp is None:
        kp = vp = torch.zeros((H, max(T0, 1), D), dtype=dk.dtype, device="cuda")
    assert kp.shape == vp.shape == (H, max(T0, 1), D)
    return types.SimpleNamespace(B=B, H=H, T0=T0, lens=lens, qkv=qkv, dk=dk, dv=dv, kp=kp.contiguous(),
                                 vp=vp.contiguous(), fp8=fp8, rows=rows,
                                 fmt=_lib.NS_KV_FP8 if fp8 else _lib.NS_KV_FP16)


def _slice(s, a, b, C=1):
    return _state(b - a, s.H, s.T0, s.lens[a:b], s.qkv[a * C:b * C], s.dk[a:b], s.dv[a:b], s.kp, s.vp, s.fp8)


def _prefix_args(s):
    return (s.kp.data_ptr() if s.T0 else None, s.vp.data_ptr() if s.T0 else None, s.kp.stride(0) if s.T0 else 0, s.T0)


def _new_rows(s, C=1):
    """The new tokens' k and v as the cache stores them, [B * C, H, D]."""
    x = s.qkv.view(-1, 3, s.H, D)
    k, v = x[:, 1].contiguous(), x[:, 2].contiguous()
    return (_q8(k), _q8(v)) if s.fp8 else (k, v)


def _appended(s, C=1, rows=None):
    """dk / dv with the C new rows of every stream in place (what a correct append leaves behind)."""
    kn, vn = rows if rows is not None else _new_rows(s, C)
    k, v = s.dk.clone(), s.dv.clone()
    bi = torch.arange(s.B, device="cuda")
    for i in range(C):
        r = torch.from_numpy(s.lens - s.T0 + i).cuda()
        k[bi, :, r] = kn.view(s.B, C, s.H, D)[:, i]
        v[bi, :, r] = vn.view(s.B, C, s.H, D)[:, i]
    return k, v


def _lockstep(s, scale=SCALE):
    """ns_decode_attention_fp8 / _prefix on streams of one length: (out, k cache, v cache after the call)."""
    L0 = int(s.lens[0])
    assert (s.lens == L0).all() and L0 - s.T0 < s.rows
    k, v = s.dk.clone(), s.dv.clone()
    out = torch.full((s.B, s.H * D), 7.0, device="cuda").half()
    f = _lib.lib().ns_decode_attention_fp8 if s.fp8 else _lib.lib().ns_decode_attention_prefix
    rc = f(s.qkv.data_ptr(), s.qkv.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), 0,
           *_prefix_args(s), s.B, s.H, D, L0, None, s.T0 + s.rows, 0, out.data_ptr(), out.stride(0), scale,
           _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out, k, v


def _lockstep_slices(s, scale=SCALE, step=None):
    """The lockstep kernel's one-pair-per-workgroup form: launches of at most 1,024 pairs."""
    step = step or 1024 // s.H
    parts = [_lockstep(_slice(s, a, min(a + step, s.B)), scale) for a in range(0, s.B, step)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


class Pool:
    """The streams' rows scattered over 32-row pages in random order; every byte outside this layer's mapped blocks
    (the other layer, three spare pages) is random filler that must survive the launches."""

    def __init__(self, s, seed):
        self.s, self.nch = s, s.rows // 32
        g = torch.Generator(device="cuda").manual_seed(seed)
        npages = s.B * self.nch + 3
        self.base = _rand_cache((npages, NLAYER, 2, s.H, 32, D), g, s.fp8)
        self.perm = np.random.default_rng(seed).permutation(npages)[: s.B * self.nch].reshape(s.B, self.nch)
        self.pool = self.image(s.dk, s.dv)
        page_bytes = self.pool[0].numel() * self.pool.element_size()
        table = np.zeros((s.B, self.nch + 1), dtype=np.int64)  # the entry after a stream's last page stays 0
        table[:, : self.nch] = self.pool.data_ptr() + self.perm * page_bytes
        self.table = torch.from_numpy(table).cuda()

    def image(self, dk, dv):
        """The whole pool as it must look when the streams' rows are dk / dv."""
        s, idx = self.s, torch.from_numpy(self.perm).cuda()
        pool = self.base.clone()
        pool[idx, LAYER, 0] = dk.view(s.B, s.H, self.nch, 32, D).permute(0, 2, 1, 3, 4)
        pool[idx, LAYER, 1] = dv.view(s.B, s.H, self.nch, 32, D).permute(0, 2, 1, 3, 4)
        return pool

    def pages_of(self, b):
        return torch.from_numpy(self.perm[b]).cuda()


def _paged(s, p, scale=SCALE, a=0, b=None):
    """ns_decode_attention_paged on streams a .. b - 1 (a row range of the table is a table)."""
    b = s.B if b is None else b
    out = torch.full((b - a, s.H * D), 7.0, device="cuda").half()
    lens = torch.from_numpy(s.lens[a:b].astype(np.int32)).cuda()
    tab, qkv = p.table[a:b], s.qkv[a:b]
    rc = _lib.lib().ns_decode_attention_paged(
        qkv.data_ptr(), qkv.stride(0), tab.data_ptr(), tab.stride(0), tab.shape[1], LAYER * 2 * s.H * 32 * D,
        *_prefix_args(s), b - a, s.H, D, lens.data_ptr(), 0, s.fmt, None, 0, None, out.data_ptr(), out.stride(0),
        scale, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _paged_slices(s, p, scale=SCALE):
    """The paged kernel's one-pair-per-workgroup form: launches of at most 1,024 pairs."""
    step = 1024 // s.H
    return torch.cat([_paged(s, p, scale, a, min(a + step, s.B)) for a in range(0, s.B, step)])


def _chunk(s, p, C, scale=SCALE):
    """ns_decode_attention_paged_chunk, every stream C new rows: out [B * C, H D]."""
    out = torch.full((s.B * C, s.H * D), 7.0, device="cuda").half()
    lens = torch.from_numpy(s.lens.astype(np.int32)).cuda()
    cnt = torch.full((s.B,), C, dtype=torch.int32, device="cuda")
    rc = _lib.lib().ns_decode_attention_paged_chunk(
        s.qkv.data_ptr(), s.qkv.stride(0), p.table.data_ptr(), p.table.stride(0), p.table.shape[1],
        LAYER * 2 * s.H * 32 * D, *_prefix_args(s), s.B, s.H, D, lens.data_ptr(), 0, s.fmt, C, cnt.data_ptr(),
        out.data_ptr(), out.stride(0), scale, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _mismatches(got, want):
    return int((got.contiguous().view(torch.uint8) != want.contiguous().view(torch.uint8)).sum())


# ------------------------------------------------------------------------------------------ (a) the quantiser
def test_quantiser_equals_the_integer_reference_on_every_fp16_pattern():
    bits, want = fc.quantiser_case()
    got = _q8(fc.f16_tensor(bits, "cuda")).cpu().numpy()
    nan = np.isnan(bits.view(np.float16))
    wrong = int((got[~nan] != want[~nan]).sum())
    lost = int((~fc.is_nan_byte(got[nan])).sum())
    print(f"quantiser: {wrong} of {int((~nan).sum())} non-NaN values differ from the reference; {lost} of "
          f"{int(nan.sum())} NaN inputs gave no NaN byte (bytes seen: {sorted(set(got[nan].tolist()))})")
    assert wrong == 0
    assert lost == 0


# --------------------------------------------------------------------------- (b) every append site = the quantiser
SITE_H, SITE_TOKENS = 2, 520  # 1,040 (token, head) rows: every pattern through k and through v, 16 rows twice


def _site_qkv():
    bits, _, _ = fc.append_site_qkv(SITE_TOKENS, SITE_H, seed=3)
    return fc.f16_tensor(bits, "cuda"), fc.nonfinite_tokens(SITE_TOKENS, SITE_H)


def _site_state(B, T0, lens, C=1, seed=0):
    qkv, bad = _site_qkv()
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    lens = np.broadcast_to(np.asarray(lens), (B,))
    rows = (int(lens.max()) - T0 + C + 31) // 32 * 32
    dk, dv = (fc.random_finite_bytes((B, SITE_H, rows, D), g, "cuda") for _ in range(2))
    kp, vp = (fc.random_finite_bytes((SITE_H, max(T0, 1), D), g, "cuda") for _ in range(2))
    return _state(B, SITE_H, T0, lens, qkv[: B * C], dk, dv, kp, vp), bad[: B * C]


def _check_site(s, bad, out, k, v, C=1):
    want_k, want_v = _appended(s, C)
    print(f"append site: {_mismatches(k, want_k)} K and {_mismatches(v, want_v)} V bytes differ from the quantiser's")
    assert _same(k, want_k) and _same(v, want_v)
    fin = torch.from_numpy(~bad).cuda()
    assert bool(torch.isfinite(out[fin]).all())  # the non-finite patterns sit in streams of their own


def test_site_rows_quantise_to_the_reference():
    """What (b) compares with: ns_quantize_fp8 of the k / v rows is the reference's bytes (NaN: a NaN byte)."""
    bits, kb, vb = fc.append_site_qkv(SITE_TOKENS, SITE_H, seed=3)
    s, _ = _site_state(SITE_TOKENS, 0, 3)
    for got, pat in zip(_new_rows(s), (kb, vb)):
        got, want = got.cpu().numpy(), fc.e4m3fn_from_f16_bits(pat)
        nan = np.isnan(pat.view(np.float16))
        assert np.array_equal(got[~nan], want[~nan]) and fc.is_nan_byte(got[nan]).all()


@pytest.mark.parametrize("B,T0", [(512, 0), (520, 0), (520, 7)])  # 1,024 pairs: one per workgroup; 1,040: eight
def test_append_lockstep_stores_the_quantisers_bytes(B, T0):
    s, bad = _site_state(B, T0, T0 + 3, seed=B + T0)
    out, k, v = _lockstep(s)
    _check_site(s, bad, out, k, v)


@pytest.mark.parametrize("B,T0,hi", [(520, 32, 255),   # eight pairs per workgroup, every key count <= 256: short path
                                     (520, 7, 255),    # no whole context chunk: the general path
                                     (520, 32, 290),   # split pairs among them: their workgroups leave the short path
                                     (512, 0, 290)])   # one pair per workgroup
def test_append_paged_stores_the_quantisers_bytes(B, T0, hi):
    lens = np.random.default_rng(B + T0 + hi).integers(T0, hi, size=B)
    lens[:4] = [T0, T0 + 31, T0 + 32, hi - 1]
    s, bad = _site_state(B, T0, lens, seed=B + T0 + hi)
    p = Pool(s, seed=hi)
    out = _paged(s, p)
    want = p.image(*_appended(s))
    print(f"paged append: {_mismatches(p.pool, want)} pool bytes differ")
    assert _same(p.pool, want)  # the append, the quantiser's bytes, and nothing else in the pool
    assert bool(torch.isfinite(out[torch.from_numpy(~bad).cuda()]).all())


@pytest.mark.parametrize("C,T0", [(1, 7), (4, 0), (4, 40)])
def test_append_chunk_stores_the_quantisers_bytes(C, T0):
    B = SITE_TOKENS // C  # C = 4: the 16 non-finite tokens are streams 124 .. 127, whole
    lens = np.random.default_rng(C + T0).integers(T0, 290, size=B)
    lens[:4] = [T0, T0 + 30, 254, T0 + 61]  # the chunk crosses a page boundary and the first split threshold
    s, bad = _site_state(B, T0, lens, C=C, seed=C + T0)
    assert bad.reshape(B, C).all(axis=1).sum() * C == bad.sum()
    p = Pool(s, seed=C)
    out = _chunk(s, p, C)
    want = p.image(*_appended(s, C))
    print(f"chunk append C={C}: {_mismatches(p.pool, want)} pool bytes differ")
    assert _same(p.pool, want)
    assert bool(torch.isfinite(out[torch.from_numpy(~bad).cuda()]).all())


def test_append_ragged_prefill_stores_the_quantisers_bytes():
    """ns_seq_attention_ragged with fp8 pages: sequences of 100 + 33 + 123 + 240 finite tokens, the 16 non-finite
    tokens as a sequence of their own, 8 more finite ones.  (The attention itself runs on the fp16 rows, where 65,504
    is a legal v: its rows are compared with the launch without pages, not asked to be finite.)"""
    H, lens = SITE_H, [100, 33, 123, 240, 16, 8]
    qkv, bad = _site_qkv()
    seq_start, blocks = ragged_blocks(lens)
    assert int(seq_start[-1]) == SITE_TOKENS and bad[496:512].all() and bad.sum() == 16
    ds, db = torch.from_numpy(seq_start).cuda(), torch.from_numpy(blocks).cuda()
    need = [-(-T // 32) for T in lens]
    rng = np.random.default_rng(9)
    g = torch.Generator(device="cuda").manual_seed(9)
    npages = sum(need) + 3
    pool = fc.random_finite_bytes((npages, NLAYER, 2, H, 32, D), g, "cuda")
    want = pool.clone()
    page_bytes = pool[0].numel()
    perm = rng.permutation(npages)
    n_slots = len(lens) + 2
    slots = rng.permutation(n_slots)[: len(lens)]
    table = np.zeros((n_slots, max(need) + 1), dtype=np.int64)
    kn, vn = _q8(qkv.view(-1, 3, H, D)[:, 1].contiguous()), _q8(qkv.view(-1, 3, H, D)[:, 2].contiguous())
    k = 0
    for s, T in enumerate(lens):
        a = int(seq_start[s])
        for c in range(need[s]):
            pg = int(perm[k])
            k += 1
            table[slots[s], c] = pool.data_ptr() + pg * page_bytes
            r0, r1 = 32 * c, min(32 * c + 32, T)
            want[pg, LAYER, 0, :, : r1 - r0] = kn[a + r0:a + r1].transpose(0, 1)
            want[pg, LAYER, 1, :, : r1 - r0] = vn[a + r0:a + r1].transpose(0, 1)
    tab, slot = torch.from_numpy(table).cuda(), torch.from_numpy(slots.astype(np.int32)).cuda()

    def run(with_pages):
        out = torch.full((SITE_TOKENS, H * D), 7.0, device="cuda").half()
        rc = _lib.lib().ns_seq_attention_ragged(
            qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), ds.data_ptr(), len(lens), SITE_TOKENS,
            db.data_ptr(), blocks.shape[0], H, D, SCALE, tab.data_ptr() if with_pages else None, tab.stride(0),
            tab.shape[1], slot.data_ptr(), n_slots, LAYER * 2 * H * 32 * D, _lib.NS_KV_FP8, _stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        return out

    filler = pool.clone()
    alone = run(False)
    assert _same(pool, filler)  # no table: nothing stored
    out = run(True)
    print(f"ragged page store: {_mismatches(pool, want)} pool bytes differ")
    assert _same(pool, want)
    assert _same(out, alone)  # the store does not touch the attention
    fin = torch.from_numpy(~bad).cuda()
    assert not bool(torch.isnan(out[fin]).any())  # a NaN row stays inside its own sequence


# ------------------------------------------------------------------------------- (c), (d) the dequantiser sweeps
def _sweep_state(case, B, H, seed=0):
    """The byte sweeps' one cached row per pair (stream row 0) plus the new token; the other rows of the page are
    random non-NaN filler, never attended."""
    T0 = case["T0"]
    n = B * H
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.stack([fc.f16_tensor(case[x][:n], "cuda").view(B, H, D) for x in ("q", "k_new", "v_new")], dim=1)
    dk, dv = (fc.random_finite_bytes((B, H, 32, D), g, "cuda") for _ in range(2))
    dk[:, :, 0] = fc.byte_tensor(case["k_row"][:n], "cuda").view(B, H, D)
    dv[:, :, 0] = fc.byte_tensor(case["v_row"][:n], "cuda").view(B, H, D)
    kp = fc.byte_tensor(np.broadcast_to(case["k_pre"], (H, D)), "cuda")[:, None, :].expand(H, max(T0, 1), D)
    vp = fc.byte_tensor(np.broadcast_to(case["v_pre"], (H, D)), "cuda")[:, None, :].expand(H, max(T0, 1), D)
    return _state(B, H, T0, T0 + 1, qkv.reshape(B, 3 * H * D).contiguous(), dk, dv, kp, vp)


SWEEP_KERNELS = {  # name -> (T0, how to run a state; returns the output rows)
    "lockstep, one pair per workgroup": (0, lambda s: _lockstep_slices(s, 1.0)[0]),
    "lockstep, eight pairs": (0, lambda s: _lockstep(s, 1.0)[0]),
    "lockstep, eight pairs, prefix": (7, lambda s: _lockstep(s, 1.0)[0]),
    "paged, short path": (32, lambda s: _paged(s, Pool(s, 1), 1.0)),
    "paged, general path": (7, lambda s: _paged(s, Pool(s, 2), 1.0)),
    "paged, one pair per workgroup": (0, lambda s: _paged_slices(s, Pool(s, 3), 1.0)),
    "chunk, C = 1": (0, lambda s: _chunk(s, Pool(s, 4), 1, 1.0)),
}


@pytest.mark.parametrize("kernel", list(SWEEP_KERNELS))
def test_v_dequantiser_returns_every_byte_at_every_dim_exactly(kernel):
    T0, run = SWEEP_KERNELS[kernel]
    B, H = 520, 2  # 1,040 pairs (eight per workgroup where the kernel has that form): the 256 Latin rows four times
    case = fc.v_sweep_case(B * H, T0)
    out = run(_sweep_state(case, B, H)).double().view(B * H, D).cpu().numpy()
    want = case["want"]
    nan = np.isnan(want)
    wrong = int((out[~nan] != want[~nan]).sum())  # (values: -0 == +0, the sign of zero is not asserted)
    print(f"V sweep, {kernel}: {wrong} of {int((~nan).sum())} elements differ from deq(byte); "
          f"{int(np.isnan(out).sum())} NaN outputs for {int(nan.sum())} NaN bytes")
    assert wrong == 0
    assert np.array_equal(np.isnan(out), nan)  # a NaN byte: NaN in that element only


@pytest.mark.parametrize("kernel", list(SWEEP_KERNELS))
def test_k_dequantiser_scores_every_byte_at_every_dim(kernel):
    T0, run = SWEEP_KERNELS[kernel]
    H = 2
    case = fc.k_sweep_case(H, T0, pre_dim=[63, 0])
    B = case["byte"].size // H
    out = run(_sweep_state(case, B, H)).double().view(B * H, D).cpu().numpy()
    want = case["want"]
    nan = np.isnan(want)
    assert nan.sum() == 2 * D
    err = np.abs(out[~nan, 0] - want[~nan])
    i = int(np.argmax(err))
    print(f"K sweep, {kernel}: max err/tol = {err.max() / fc.K_TOL:.4f} (byte 0x{case['byte'][~nan][i]:02X} at dim "
          f"{case['dim'][~nan][i]})")
    assert np.isfinite(out[~nan]).all()
    assert (err <= fc.K_TOL).all()
    assert (out[~nan, 1:] == 0).all()  # cached v = e0, new v = 0
    assert np.isnan(out[nan]).all()  # a NaN byte in the key: the score, the softmax and the whole row are NaN


# ------------------------------------------------------------------------- (e) heavy-tailed attention vs float64
def _heavy_case(B, H, T0, L0, rows=None, seed=0):
    c = fc.heavy_tail(build_case(B, H, T0, L0, np.full((B, H), -1), rows=rows, seed=seed, device="cuda", probe=False))
    return to_fp8(c, _q8)


def _check_heavy(c, out, name, streams=None):
    """check_output of tests/test_gpu_attention_probes.py without its probe-dominates assertion (there is no probe
    here): the same float64 reference, the same tolerance()."""
    bs = torch.arange(c.B) if streams is None else torch.as_tensor(streams)
    want, vmax = attention_ref(c, torch.float64, bs)
    ref32, _ = attention_ref(c, torch.float32, bs)
    tol = tolerance(want, ref32, vmax)
    err = (out.double().view(-1, c.H, D) - want).abs()
    ratio = float((err / tol).max())
    print(f"{name}: max err/tol = {ratio:.4f} (max err {float(err.max()):.3e}, max |v| {vmax:.0f})")
    assert bool(torch.isfinite(out).all())
    assert bool((err <= tol).all()), (name, ratio)
    return ratio


@pytest.mark.parametrize("Lk,T0", [(65, 0), (513, 32), (1100, 0)])  # one, four and eight waves a pair
def test_heavy_tailed_attention_lockstep(Lk, T0):
    B, H = 92, 12
    c = _heavy_case(B, H, T0, Lk - 1, seed=3 * Lk + T0)
    _check_heavy(c, _launch(c), f"heavy fp8 lockstep Lk={Lk} T0={T0}")


@pytest.mark.parametrize("B,T0", [(22, 7), (110, 32)])  # one pair and eight pairs per workgroup; every split class
def test_heavy_tailed_attention_paged(B, T0):
    H = 12
    Lk = _paged_lengths(B, T0)
    L0 = Lk - 1
    nch = int((L0.max() - T0) // 32 + 1)
    c = _heavy_case(B, H, T0, L0, rows=nch * 32, seed=B + T0)
    s = _state(B, H, T0, L0, c.qkv, c.ks, c.vs, c.kp, c.vp)
    p = Pool(s, seed=B)
    out = _paged(s, p)
    assert _same(p.pool, p.image(*_appended(s)))
    worst = 0.0
    for v in sorted(set(L0.tolist())):  # streams of one length share a reference
        bs = np.nonzero(L0 == v)[0]
        worst = max(worst, _check_heavy(c, out[torch.from_numpy(bs).cuda()], f"heavy fp8 paged B={B} T0={T0} "
                                        f"Lk={v + 1}", streams=bs))
    print(f"heavy fp8 paged B={B} T0={T0}: max err/tol = {worst:.4f}")


# --------------------------------------------------------------------- (f) same bits on caches of full-range bytes
def _heavy_qkv(B, H, seed):
    g = torch.Generator().manual_seed(seed)
    c = types.SimpleNamespace(B=B, H=H, qkv=torch.randn((B, 3 * H * D), generator=g).half().cuda())
    c.kp = c.ks = c.vp = c.vs = torch.zeros((1, D), device="cuda").half()  # (only the new token is scaled here)
    return fc.heavy_tail(c).qkv


@pytest.mark.parametrize("T0,hi", [(32, 255), (7, 300)])  # the short path; the general path with split pairs
def test_paged_equals_lockstep_on_full_range_bytes(T0, hi):
    B, H = 90, 12
    g = torch.Generator(device="cuda").manual_seed(T0 + hi)
    lens = np.random.default_rng(T0 + hi).integers(T0, hi, size=B)
    lens[:5] = [T0, T0 + 31, T0 + 32, T0 + 63, hi - 1]
    rows = (int(lens.max()) - T0) // 32 * 32 + 32
    dk, dv = (fc.random_finite_bytes((B, H, rows, D), g, "cuda") for _ in range(2))
    kp, vp = (fc.random_finite_bytes((H, T0, D), g, "cuda") for _ in range(2))
    s = _state(B, H, T0, lens, _heavy_qkv(B, H, seed=hi), dk, dv, kp, vp)
    p = Pool(s, seed=hi)
    out = _paged(s, p)
    assert bool(torch.isfinite(out).all())
    ref = [_lockstep(_slice(s, b, b + 1)) for b in range(B)]  # every stream alone, none sampled
    assert _same(out, torch.cat([r[0] for r in ref]))
    assert _same(p.pool, p.image(torch.cat([r[1] for r in ref]), torch.cat([r[2] for r in ref])))


@pytest.mark.parametrize("T0", [0, 40])
def test_chunk_equals_one_token_kernel_on_full_range_bytes(T0):
    """C = 5 from 30 own rows (the page boundary inside the chunk) and from L = 254 (the first split threshold), with
    the comparison of tests/test_gpu_attention_chunk.py: outputs and every pool byte, bit for bit."""
    c = chunk_tests._build("fp8", 5, T0, [T0 + 30, 254], seed=800 + T0)
    g = torch.Generator(device="cuda").manual_seed(T0)
    c["pool"].copy_(fc.random_finite_bytes(tuple(c["pool"].shape), g, "cuda"))  # in place: the table holds addresses
    c["kp"], c["vp"] = (fc.random_finite_bytes(tuple(c["kp"].shape), g, "cuda") for _ in range(2))
    c["qkv"] = _heavy_qkv(c["B"] * 5, chunk_tests.H, seed=T0)
    chunk_tests._compare(c, [5, 5])


# ------------------------------------------------------------------------------ (g) a poisoned stream stays poisoned
def _two_steps(kv, B, H, T0, lens, paged, poison):
    """Two consecutive decode steps; in the first, stream ``poison`` (if not None) has an all-NaN qkv row.  Returns
    [(out, k rows, v rows) after step 1, after step 2], the rows as dense [B, H, rows, D] plus, for the paged kernel,
    the whole pool."""
    fp8 = kv == "fp8"
    g = torch.Generator(device="cuda").manual_seed(B + T0)
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (B,))
    rows = (int(lens.max()) - T0 + 2 + 31) // 32 * 32
    dk, dv = (_rand_cache((B, H, rows, D), g, fp8) for _ in range(2))
    kp, vp = (_rand_cache((H, max(T0, 1), D), g, fp8) for _ in range(2))
    qkv = [torch.randn((B, 3 * H * D), generator=g, device="cuda").half() for _ in range(2)]
    if poison is not None:
        qkv[0][poison] = float("nan")
    res = []
    if paged:
        s = _state(B, H, T0, lens, qkv[0], dk, dv, kp, vp, fp8)
        p = Pool(s, seed=B)
        for i in range(2):
            s.qkv, s.lens = qkv[i], lens + i
            res.append((_paged(s, p), p.pool.clone()))
        return res, p
    for i in range(2):
        out, dk, dv = _lockstep(_state(B, H, T0, lens + i, qkv[i], dk, dv, kp, vp, fp8))
        res.append((out, torch.stack([dk, dv])))
    return res, None


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("kernel,B,H,T0", [("lockstep", 6, 2, 0), ("lockstep", 90, 12, 7),
                                           ("paged", 6, 12, 0), ("paged", 90, 12, 32)])
def test_a_poisoned_stream_stays_poisoned(kv, kernel, B, H, T0):
    paged = kernel == "paged"
    bad = 3
    lens = T0 + 5
    if paged:
        lens = np.random.default_rng(B).integers(T0, 254, size=B)
        lens[:6] = [T0, T0 + 5, T0 + 30, T0 + 31, T0 + 63, 253]  # stream 3: its two rows lie in two pages
    clean, _ = _two_steps(kv, B, H, T0, lens, paged, None)
    dirty, p = _two_steps(kv, B, H, T0, lens, paged, bad)
    others = torch.arange(B, device="cuda") != bad
    for i in range(2):
        assert bool(torch.isfinite(clean[i][0]).all())
        n_nan = int(torch.isnan(dirty[i][0][bad]).sum())
        print(f"{kv} {kernel} step {i + 1}: {n_nan} of {H * D} outputs of the poisoned stream are NaN")
        assert _same(dirty[i][0][others], clean[i][0][others])  # the other streams: the same bits
        if paged:
            a, b = dirty[i][1].clone(), clean[i][1]
            a[p.pages_of(bad)] = b[p.pages_of(bad)]
            assert _same(a, b)  # every pool byte outside the poisoned stream's pages
        else:
            assert _same(dirty[i][1][:, others], clean[i][1][:, others])
    assert bool(torch.isnan(dirty[0][0][bad]).all())  # step 1: its q is NaN
    assert bool(torch.isnan(dirty[1][0][bad]).all())  # step 2: finite qkv, but the row it stored is still NaN
