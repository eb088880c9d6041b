"""GPU: one-hot position probes for the attention kernels (csrc/nsg_attn.hip).

The other reference tests draw q/k/v from N(0, 1): the softmax is then near-uniform, every output is about
1/sqrt(Lk), and a key wrongly dropped or included at Lk ~ 1,000 moves the output by ~1e-3 -- inside their flat 2e-3
tolerance.  Here every (stream, head) pair gets one PROBE position j whose key is a spike for the pair's own query,

    k[j] = q * c / (|q|^2 * scale),  c = 30  (natural-log units),   v[j] = a fresh N(0, 1) row,

so that the softmax weight of j is >= 1 - 1e-9 and the expected output is v[j]: an error at that position is O(1).
Every row the kernel must NOT use (rows past L0, the stale content of row L0 before the call, rows before the window
start) carries a finite POISON, k = q * 60 / (|q|^2 * scale), v = 100: if one of them enters the softmax the output
is about 100.  Both are finite in fp16 and in e4m3, so no NaN semantics are involved.

Reference: float64 torch softmax(q k^T * scale) v over exactly the attended rows [s0, L0] (the dequantised bytes for
the fp8 cache, the new token's k/v quantised with ns_quantize_fp8).  Tolerance, nothing tuned to the kernel:

    tol = 2^-10 |want| + 8 max|ref32 - ref64| + 2^-20 max|v|        (+ 2^-10 (P @ |v|) for ns_seq_attention)

2^-10 = twice the half-ulp of the fp16 output; ref32 = the same formula in plain float32 torch (the kernel is fp32 with
another summation order and exp2, hence the 8); the last term is a floor for when fp32 and fp64 agree exactly; the
sequence kernel rounds P to fp16 before the PV product (half-ulp 2^-11 per term, doubled).

The probe builder and the references are pure torch and run on any device: tests/test_attention_probes_host.py
checks on the CPU that the probes see the off-by-one errors the N(0, 1) tests cannot.

A prefix row is shared by every stream, so it can be the spike of one pair only: where two pairs ask for the same
prefix row the later one probes the new token (position L0) instead; every position keeps its first claimant.  The
other streams of that head see the spike as well, at a random score: the owner's q is doubled so that it stays far
enough below 30 for the references' own check (|want - v[j]| < 1e-6) to hold; everything else is the usual N(0, 1).
"""

import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402

pytestmark = pytest.mark.gpu

D = 64
SCALE = D ** -0.5
C_PROBE, C_POISON, V_POISON = 30.0, 60.0, 100.0


# ----------------------------------------------------------------------------------------------- probe builder
def spike(q, c):
    """fp16 key with q . k * scale = c (up to the fp16 rounding of k)."""
    qf = q.float()
    return (qf * (c / (qf.pow(2).sum(-1, keepdim=True) * SCALE))).half()


def quant_torch(t):
    """OCP e4m3fn bytes of an fp16 tensor, saturated (what ns_quantize_fp8 computes; CPU stand-in)."""
    return t.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant(u):
    return u.view(torch.float8_e4m3fn).float()


def build_case(B, H, T0, L0, pos, rows=None, window=0, seed=0, device="cpu", probe=True):
    """Decode-step inputs with probes and poison.

    L0: cached positions, an int or one per stream.  pos: [B, H] probe positions in [s0, L0] (-1: none).
    The stream cache holds ``rows`` rows (positions T0 .. T0 + rows - 1; default L0 + 4 - T0).  probe=False gives
    the plain N(0, 1) inputs of the older tests (no spike, no poison).  q and the probe rows come from a CPU generator
    (the same on every device); the bulk N(0, 1) rows from the device's."""
    L0 = torch.as_tensor(L0, dtype=torch.long).reshape(-1).expand(B).clone()
    assert int(L0.min()) >= T0
    rows = rows or int(L0.max()) + 4 - T0
    assert rows > int(L0.max()) - T0
    gc = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B, 3 * H * D), generator=gc).half().to(device)
    vprobe = torch.randn((B, H, D), generator=gc).half().to(device)
    gd = torch.Generator(device=device).manual_seed(seed + 1000003)  # another sequence than gc's on the CPU too
    kp = torch.randn((H, max(T0, 1), D), generator=gd, device=device).half()
    vp = torch.randn((H, max(T0, 1), D), generator=gd, device=device).half()
    ks = torch.randn((B, H, rows, D), generator=gd, device=device).half()
    vs = torch.randn((B, H, rows, D), generator=gd, device=device).half()
    x = qkv.view(B, 3, H, D)
    q = x[:, 0]
    s0 = (L0 + 1 - window).clamp(min=0) if window > 0 else torch.zeros_like(L0)
    pos = torch.as_tensor(np.asarray(pos), dtype=torch.long).reshape(B, H).clone()
    if probe:
        assert bool(((pos < 0) | ((pos >= s0[:, None]) & (pos <= L0[:, None]))).all())
        # a prefix row serves one pair: later claimants probe the new token instead
        pre = (pos >= 0) & (pos < T0)
        bi, hi = pre.nonzero(as_tuple=True)
        if len(bi):
            key = (hi * max(T0, 1) + pos[bi, hi]).numpy()
            first = np.zeros(len(key), dtype=bool)
            first[np.unique(key, return_index=True)[1]] = True
            lose = torch.from_numpy(~first)
            pos[bi[lose], hi[lose]] = L0[bi[lose]]
            bi, hi = bi[~lose], hi[~lose]
            # ... and every other stream of the head sees that spike too, at a score of 30 (q' . q) / |q|^2 ~
            # N(0, (30 / |q|)^2): with |q| ~ 8 a 4-sigma stream would put 1e-6 of it into its own reference.  The
            # owner's q is doubled (its spike halves, the foreign scores with it; its own scores stay far below 30)
            x[:, 0][bi.to(device), hi.to(device)] *= 2
        pk = spike(q, C_POISON)
        r = torch.arange(rows, device=device)[None, None, :] + T0
        bad = ((r >= L0.to(device)[:, None, None]) | (r < s0.to(device)[:, None, None]))[..., None]  # [B, 1, rows, 1]
        ks = torch.where(bad, pk[:, :, None, :], ks)
        vs = torch.where(bad, torch.full_like(vs[:1, :1, :1, :1], V_POISON), vs)
        s0min = int(s0.min())
        if min(s0min, T0) > 0:  # prefix rows before the window start: one stream's poison each (the row is shared)
            assert int(s0.max()) == s0min
            hh = torch.arange(H, device=device)
            for rr in range(min(s0min, T0)):
                kp[:, rr] = pk[(rr * 7 + hh) % B, hh]
                vp[:, rr] = V_POISON
        sk = spike(q, C_PROBE)
        bi, hi = ((pos >= 0) & (pos < T0)).nonzero(as_tuple=True)
        if len(bi):
            kp[hi.to(device), pos[bi, hi].to(device)] = sk[bi.to(device), hi.to(device)]
            vp[hi.to(device), pos[bi, hi].to(device)] = vprobe[bi.to(device), hi.to(device)]
        m_new = (pos == L0[:, None]).to(device)
        x[:, 1][m_new] = sk[m_new]
        x[:, 2][m_new] = vprobe[m_new]
        bi, hi = ((pos >= T0) & (pos < L0[:, None])).nonzero(as_tuple=True)
        if len(bi):
            jj = (pos[bi, hi] - T0).to(device)
            ks[bi.to(device), hi.to(device), jj] = sk[bi.to(device), hi.to(device)]
            vs[bi.to(device), hi.to(device), jj] = vprobe[bi.to(device), hi.to(device)]
    else:
        pos.fill_(-1)
    return types.SimpleNamespace(B=B, H=H, T0=T0, L0=L0, s0=s0, window=window, rows=rows, cap=T0 + rows, pos=pos,
                                 qkv=qkv, vprobe=vprobe, kp=kp, vp=vp, ks=ks, vs=vs, fp8=False,
                                 quant=lambda t: t, deq=lambda t: t.float())


def to_fp8(c, quant):
    """The same case over an e4m3 cache: prefix and stream rows as bytes; the new token stays fp16 in qkv."""
    c.kp, c.vp, c.ks, c.vs = quant(c.kp), quant(c.vp), quant(c.ks), quant(c.vs)
    c.fp8, c.quant, c.deq = True, quant, dequant
    return c


def new_kv(c):
    x = c.qkv.view(c.B, 3, c.H, D)
    return c.quant(x[:, 1].contiguous()), c.quant(x[:, 2].contiguous())


def attention_ref(c, dtype, streams=None, rows=None, stale=False):
    """softmax(q k^T * scale) v in ``dtype`` over positions ``rows`` (default: the attended rows [s0, L0]) of the
    streams ``streams`` (default all; they must share L0 and s0).  Row L0 is the new token's k/v unless ``stale``
    (then the cache's content before the call: one of the deliberately wrong variants)."""
    bs = torch.arange(c.B) if streams is None else torch.as_tensor(streams)
    L0, s0 = int(c.L0[bs[0]]), int(c.s0[bs[0]])
    assert bool((c.L0[bs] == L0).all()) and bool((c.s0[bs] == s0).all())
    dev = c.qkv.device
    bd = bs.to(dev)
    kk, vv = c.deq(c.ks[bd]), c.deq(c.vs[bd])
    if c.T0:
        kk = torch.cat([c.deq(c.kp)[None, :, :c.T0].expand(len(bs), -1, -1, -1), kk], dim=2)
        vv = torch.cat([c.deq(c.vp)[None, :, :c.T0].expand(len(bs), -1, -1, -1), vv], dim=2)
    if not stale:
        kn, vn = new_kv(c)
        kk[:, :, L0], vv[:, :, L0] = c.deq(kn[bd]), c.deq(vn[bd])
    idx = torch.arange(s0, L0 + 1) if rows is None else torch.as_tensor(rows)
    kk, vv = kk[:, :, idx.to(dev)].to(dtype), vv[:, :, idx.to(dev)].to(dtype)
    q = c.qkv.view(c.B, 3, c.H, D)[bd, 0].to(dtype)
    s = torch.einsum("bhd,bhjd->bhj", q, kk) * SCALE
    return torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), vv), float(vv.abs().max())


def tolerance(want64, ref32, vmax):
    return 2.0 ** -10 * want64.abs() + 8.0 * (ref32.double() - want64).abs().max() + 2.0 ** -20 * vmax


def expected_probe_rows(c):
    """v[j] as the kernel sees it ([B, H, D] float64)."""
    return c.deq(c.quant(c.vprobe)).double()


def reference_and_tolerance(c, streams=None):
    """(want fp64 [n, H, D], tol) for the rows of ``streams``; asserts that the probe dominates the reference."""
    bs = torch.arange(c.B) if streams is None else torch.as_tensor(streams)
    want, vmax = attention_ref(c, torch.float64, bs)
    ref32, _ = attention_ref(c, torch.float32, bs)
    tol = tolerance(want, ref32, vmax)
    probed = (c.pos[bs] >= 0).to(want.device)
    sanity = (want - expected_probe_rows(c)[bs.to(want.device)]).abs().amax(-1)
    assert float(sanity[probed].max()) < 1e-6, float(sanity[probed].max())
    return want, tol


def check_output(c, out, name, streams=None):
    """out [n, H*D] (the rows of ``streams``) against the fp64 reference; prints the largest err / tol."""
    want, tol = reference_and_tolerance(c, streams)
    err = (out.double().view(-1, c.H, D) - want).abs()
    ratio = float((err / tol).max())
    print(f"{name}: max err/tol = {ratio:.4f} (max err {float(err.max()):.3e})")
    assert bool(torch.isfinite(out).all())
    assert bool((err <= tol).all()), (name, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _q8(t):
    out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    assert _lib.lib().ns_quantize_fp8(t.contiguous().data_ptr(), out.data_ptr(), t.numel(), _stream_handle()) == 0
    return out


def _case(kv, *a, **k):
    c = build_case(*a, device="cuda", **k)
    return to_fp8(c, _q8) if kv == "fp8" else c


def _launch(c, api="host"):
    """One lockstep decode step.  api: 'host' (L0 an argument), 'devptr' (L0 from device memory), 'plane' (chunk-plane
    layout), 'dev' (ns_decode_attention_dev: T0 = 0, fp16, L0 from device memory).  Checks the return code, the KV
    append and that nothing else in the cache changed; returns the output rows."""
    lib = _lib.lib()
    B, H, T0, L0 = c.B, c.H, c.T0, int(c.L0[0])
    ks, vs = c.ks.clone(), c.vs.clone()
    strides = (ks.stride(0), ks.stride(1), 0)
    if api == "plane":
        assert c.rows % 32 == 0
        ks = ks.view(B, H, c.rows // 32, 32, D).permute(2, 0, 1, 3, 4).contiguous()  # [chunk, B, H, 32, D]
        vs = vs.view(B, H, c.rows // 32, 32, D).permute(2, 0, 1, 3, 4).contiguous()
        strides = (ks.stride(1), ks.stride(2), ks.stride(0))
    out = torch.full((B, H * D), float("nan"), device="cuda").half()
    dL = torch.tensor([L0], dtype=torch.int32, device="cuda")
    if api == "dev":
        assert T0 == 0 and not c.fp8 and c.window == 0
        rc = lib.ns_decode_attention_dev(c.qkv.data_ptr(), c.qkv.stride(0), ks.data_ptr(), vs.data_ptr(), strides[0],
                                         strides[1], B, H, D, dL.data_ptr(), c.cap, out.data_ptr(), out.stride(0),
                                         SCALE, _stream_handle())
    else:
        f = lib.ns_decode_attention_fp8 if c.fp8 else lib.ns_decode_attention_prefix
        dev = api == "devptr"
        rc = f(c.qkv.data_ptr(), c.qkv.stride(0), ks.data_ptr(), vs.data_ptr(), *strides,
               c.kp.data_ptr() if T0 else None, c.vp.data_ptr() if T0 else None, c.kp.stride(0) if T0 else 0, T0, B, H,
               D, -1 if dev else L0, dL.data_ptr() if dev else None, c.cap, c.window, out.data_ptr(), out.stride(0),
               SCALE, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    if api == "plane":
        ks = ks.permute(1, 2, 0, 3, 4).reshape(B, H, c.rows, D)
        vs = vs.permute(1, 2, 0, 3, 4).reshape(B, H, c.rows, D)
    kn, vn = new_kv(c)
    want_k, want_v = c.ks.clone(), c.vs.clone()
    want_k[:, :, L0 - T0], want_v[:, :, L0 - T0] = kn, vn
    assert torch.equal(ks, want_k) and torch.equal(vs, want_v)  # the append at L0 and nothing else
    return out


def _sweep(B, H, lo, hi, offset=0):
    """Pair p probes position lo + (offset + p) mod (hi - lo + 1): every position of [lo, hi] once B*H covers it."""
    return lo + (offset + np.arange(B * H)) % (hi - lo + 1)


# ------------------------------------------------------------------------------------------------ decode cases
@pytest.mark.parametrize("T0", [0, 7, 32])  # 7: the prefix ends inside a 32-row chunk
@pytest.mark.parametrize("Lk", [257, 1100])
def test_probe_every_position_fp16_multi_pair(Lk, T0):
    """B*H = 1104 pairs > NSG_ATT_SMALL_PAIRS: eight pairs per workgroup; 2-wave (Lk = 257) and 8-wave (Lk = 1100)
    splits, every 32-row chunk boundary, the prefix / stream boundary and the new token each probed once."""
    B, H, L0 = 92, 12, Lk - 1
    c = _case("fp16", B, H, T0, L0, _sweep(B, H, 0, L0), seed=Lk + T0)
    check_output(c, _launch(c), f"fp16 P=8 Lk={Lk} T0={T0}")


@pytest.mark.parametrize("Lk,T0", [(1, 0), (2, 0), (33, 0), (256, 0), (513, 0), (1024, 0),
                                   (33, 32), (256, 32), (513, 32), (1024, 32)])  # T0 < Lk: the prefix is part of it
def test_probe_every_position_fp16_one_pair_per_workgroup(Lk, T0):
    """B*H <= 1024: one pair per workgroup (register double buffer), 1 / 2 / 4-wave splits and their edges; several
    launches over slices of positions where Lk > B*H."""
    H, L0 = 12, Lk - 1
    B = min(64, max(2, -(-Lk // H)))
    for off in range(0, Lk, B * H):
        c = _case("fp16", B, H, T0, L0, _sweep(B, H, 0, L0, off), seed=Lk + T0 + off)
        check_output(c, _launch(c), f"fp16 P=1 Lk={Lk} T0={T0} off={off}")


@pytest.mark.parametrize("T0", [0, 32])
@pytest.mark.parametrize("Lk", [65, 513, 1100])
def test_probe_every_position_fp8(Lk, T0):
    B, H, L0 = 92, 12, Lk - 1
    c = _case("fp8", B, H, T0, L0, _sweep(B, H, 0, L0), seed=3 * Lk + T0)
    check_output(c, _launch(c), f"fp8 P=8 Lk={Lk} T0={T0}")


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0,L0,W", [(32, 300, 290),     # s0 = 11: inside the prefix
                                     (32, 600, 300),     # s0 = 301: inside the stream, 2 waves
                                     (5, 1100, 1030)])   # s0 = 71: 8 waves
def test_probe_window(kv, T0, L0, W):
    """window > 0: every position of [s0, L0] probed; rows < s0 (row s0 - 1 among them) carry the poison."""
    B, H = 92, 12
    s0 = L0 + 1 - W
    c = _case(kv, B, H, T0, L0, _sweep(B, H, s0, L0), window=W, seed=L0 + W)
    assert int(c.s0[0]) == s0
    check_output(c, _launch(c), f"{kv} window T0={T0} L0={L0} W={W}")


@pytest.mark.parametrize("api,T0", [("plane", 0), ("plane", 32), ("devptr", 0), ("devptr", 32),
                                    ("dev", 0)])  # ns_decode_attention_dev has no shared prefix
def test_probe_layouts_and_device_side_length(api, T0):
    """The chunk-plane cache layout, the cache length read from device memory and ns_decode_attention_dev, each with
    every position of Lk = 257 probed (B*H = 1104).  Through ns_decode_attention_dev a length at the capacity gives
    NaN rows, an untouched cache and return code 0."""
    B, H, L0 = 92, 12, 256
    rows = 288 if api == "plane" else None  # whole 32-row chunks
    c = _case("fp16", B, H, T0, L0, _sweep(B, H, 0, L0), rows=rows, seed=7 + T0)
    check_output(c, _launch(c, api), f"fp16 {api} Lk=257 T0={T0}")
    if api == "dev":
        ks, vs = c.ks.clone(), c.vs.clone()
        out = torch.full((B, H * D), 3.0, device="cuda").half()
        dL = torch.tensor([c.cap], dtype=torch.int32, device="cuda")
        rc = _lib.lib().ns_decode_attention_dev(c.qkv.data_ptr(), c.qkv.stride(0), ks.data_ptr(), vs.data_ptr(),
                                                ks.stride(0), ks.stride(1), B, H, D, dL.data_ptr(), c.cap,
                                                out.data_ptr(), out.stride(0), SCALE, _stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        assert torch.equal(ks, c.ks) and torch.equal(vs, c.vs)


# ------------------------------------------------------------------------------------------------------- paged
PAGED_LK = [1, 2, 32, 33, 256, 257, 512, 513, 1024, 1025, 1100]


def _paged_lengths(B, T0):
    """Key counts per stream cycling over PAGED_LK (values not above T0 count the stream's own rows: a stream
    cannot be shorter than the shared prefix)."""
    lk = [PAGED_LK[b % len(PAGED_LK)] for b in range(B)]
    return np.array([v if v > T0 else T0 + v for v in lk])


def _paged_positions(B, H, T0, Lk):
    """H different probe positions per stream from the edges of its own split."""
    pos = np.zeros((B, H), dtype=np.int64)
    for b in range(B):
        L0, s0 = int(Lk[b]) - 1, 0
        S = 1 if Lk[b] <= 256 else 2 if Lk[b] <= 512 else 4 if Lk[b] <= 1024 else 8
        cand = [s0, T0 - 1, T0, T0 + 31, T0 + 32] + [s0 + 32 * w for w in range(1, S)] + \
               [s0 + 32 * w - 1 for w in range(1, S)] + [L0 - 1, L0]
        cand = list(dict.fromkeys(p for p in cand if 0 <= p <= L0))
        cand = cand[b % len(cand):] + cand[:b % len(cand)]
        extra = [p for p in ((b * 7 + 13 * i) % (L0 + 1) for i in range(4 * H)) if p not in cand]
        cand = (cand + list(dict.fromkeys(extra)))[:H]
        pos[b] = (cand + [L0] * H)[:H]  # a stream with fewer than H rows probes the new token in the other heads
    return pos


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("B", [22, 110])
@pytest.mark.parametrize("T0", [0, 7, 32])
def test_probe_paged(kv, B, T0):
    """ns_decode_attention_paged: a length per stream, pages scattered in random order over a 2-layer pool (the other
    layer's block and the unused rows of each stream's last page hold the poison), P = 1 (B = 22) and P = 8 (B = 110)
    workgroup forms.  The append lands in the stream's page and nothing else in the pool changes."""
    H, n_layer, layer = 12, 2, 1
    Lk = _paged_lengths(B, T0)
    L0 = Lk - 1
    nch = int((L0.max() - T0) // 32 + 1)
    c = _case(kv, B, H, T0, L0, _paged_positions(B, H, T0, Lk), rows=nch * 32, seed=B + T0)
    rng = np.random.default_rng(B + T0)
    need = [(int(v) - T0) // 32 + 1 for v in L0]  # pages through the new token's row
    npages = sum(need) + 3
    poison_k = c.quant(spike(c.qkv.view(B, 3, H, D)[:, 0], C_POISON))  # [B, H, D]
    poison_v = c.quant(torch.full((4,), V_POISON, device="cuda").half())[:1]  # the quantiser takes 4 values at a time
    pool = torch.empty((npages, n_layer, 2, H, 32, D), dtype=poison_v.dtype, device="cuda")
    pool[:] = poison_v
    perm = rng.permutation(npages)
    table = np.zeros((B, nch + 2), dtype=np.int64)
    page_bytes = pool[0].numel() * pool.element_size()
    owner, k = [], 0
    for b in range(B):
        for ch in range(need[b]):
            pg = int(perm[k])
            k += 1
            pool[pg, layer, 0] = c.ks[b, :, 32 * ch: 32 * ch + 32]
            pool[pg, layer, 1] = c.vs[b, :, 32 * ch: 32 * ch + 32]
            pool[pg, 1 - layer, 0] = poison_k[b][:, None, :]
            table[b, ch] = pool.data_ptr() + pg * page_bytes
            owner.append((pg, b, ch))
    tab = torch.from_numpy(table).cuda()
    lens = torch.from_numpy(L0.astype(np.int32)).cuda()
    pool0 = pool.clone()
    out = torch.full((B, H * D), float("nan"), device="cuda").half()
    rc = _lib.lib().ns_decode_attention_paged(
        c.qkv.data_ptr(), c.qkv.stride(0), tab.data_ptr(), tab.stride(0), tab.shape[1], layer * 2 * H * 32 * D,
        c.kp.data_ptr() if T0 else None, c.vp.data_ptr() if T0 else None, c.kp.stride(0) if T0 else 0, T0, B, H, D,
        lens.data_ptr(), 0, _lib.NS_KV_FP8 if c.fp8 else _lib.NS_KV_FP16, None, 0, None, out.data_ptr(),
        out.stride(0), SCALE, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    kn, vn = new_kv(c)
    for pg, b, ch in owner:
        r = int(L0[b]) - T0
        if r // 32 == ch:
            pool0[pg, layer, 0, :, r % 32] = kn[b]
            pool0[pg, layer, 1, :, r % 32] = vn[b]
    assert torch.equal(pool[:, 1 - layer], pool0[:, 1 - layer])  # the other layer's block
    assert torch.equal(pool, pool0)  # the append and nothing else
    worst = 0.0
    for v in sorted(set(L0.tolist())):  # streams of one length share a reference
        bs = np.nonzero(L0 == v)[0]
        worst = max(worst, check_output(c, out[torch.from_numpy(bs).cuda()], f"{kv} paged B={B} T0={T0} Lk={v + 1}",
                                        streams=bs))
    print(f"{kv} paged B={B} T0={T0}: max err/tol = {worst:.4f}")


# ------------------------------------------------------------------------------------------ sequence attention
SEQ_DIAGONALS = [0, 15, 16, 31, 32, 63, 64, 65, 127, 128, 198, 199]


def build_seq_case(B, T, H, seed=0, device="cpu"):
    """Whole sequences: pair (b, h) takes one diagonal j*; k[j*] is the c = 30 spike for q[j*], v[j*] a fresh row,
    and k[j* + 1], v[j* + 1] the poison for q[j*] (the first row causality must keep out)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B * T, 3 * H * D), generator=g).half().to(device)
    x = qkv.view(B, T, 3, H, D)
    jstar = torch.tensor([SEQ_DIAGONALS[p % len(SEQ_DIAGONALS)] for p in range(B * H)]).view(B, H)
    for b in range(B):
        for h in range(H):
            j = int(jstar[b, h])
            qj = x[b, j, 0, h]
            x[b, j, 1, h] = spike(qj, C_PROBE)
            if j + 1 < T:
                x[b, j + 1, 1, h] = spike(qj, C_POISON)
                x[b, j + 1, 2, h] = V_POISON
    return qkv, jstar


def seq_ref(qkv, B, T, H, dtype):
    x = qkv.to(dtype).view(B, T, 3, H, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(torch.triu(torch.ones(T, T, device=qkv.device, dtype=torch.bool), 1), float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * T, H * D), (p @ v.abs()).transpose(1, 2).reshape(B * T, H * D), \
        float(v.abs().max())


def test_probe_seq_attention_diagonals():
    """ns_seq_attention, T = 200 (four 64-row tiles, the last ragged): the diagonal key of a probed row dominates, the
    row after it is poison; all rows against the fp64 causal reference, row j* equal to v[j*]."""
    B, T, H = 2, 200, 8
    qkv, jstar = build_seq_case(B, T, H, seed=5, device="cuda")
    out = torch.full((B * T, H * D), float("nan"), device="cuda").half()
    rc = _lib.lib().ns_seq_attention(qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), B, T, H, D, SCALE,
                                     _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    want, pv, vmax = seq_ref(qkv, B, T, H, torch.float64)
    ref32, _, _ = seq_ref(qkv, B, T, H, torch.float32)
    tol = tolerance(want, ref32, vmax) + 2.0 ** -10 * pv
    err = (out.double() - want).abs()
    print(f"seq T={T}: max err/tol = {float((err / tol).max()):.4f} (max err {float(err.max()):.3e})")
    assert bool((err <= tol).all()), float((err / tol).max())
    v = qkv.view(B, T, 3, H, D)[:, :, 2].double()
    o = out.double().view(B, T, H, D)
    for b in range(B):
        for h in range(H):
            j = int(jstar[b, h])
            assert float((want.view(B, T, H, D)[b, j, h] - v[b, j, h]).abs().max()) < 1e-6
            assert bool(((o[b, j, h] - v[b, j, h]).abs() <= tol.view(B, T, H, D)[b, j, h]).all()), (b, h, j)
