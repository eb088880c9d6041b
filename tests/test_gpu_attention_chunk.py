"""GPU: ``ns_decode_attention_paged_chunk`` (C queries a stream in one launch) against ``ns_decode_attention_paged``
called once per query on a cloned page pool.

Every comparison is bit equality: the output rows, every byte of the page pool (both layers of every page, so a
stray write anywhere shows) and ``d_lens`` (not advanced).  The starting lengths put a chunk across every place the
one-token kernel changes behaviour: the page boundary, the row split 1->2, 2->4 and 4->8 (``att_split`` at 256, 512
and 1,024 keys), a stream with no own rows yet, position 0 without a prefix, and a prefix that is no multiple of 32.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402

pytestmark = pytest.mark.gpu

H, D = 2, 64
LAYER, NLAYER = 1, 2
SENTINEL = 7.0
I32MAX = np.iinfo(np.int32).max


def _q8(t):
    out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    assert _lib.lib().ns_quantize_fp8(t.contiguous().data_ptr(), out.data_ptr(), t.numel(), _stream_handle()) == 0
    return out


def _rand(shape, g, kv):
    t = torch.randn(shape, generator=g, device="cuda").half()
    return _q8(t) if kv == "fp8" else t


def _build(kv, C, T0, lens, seed):
    """Streams at ``lens`` (cached positions, >= T0) with pages through row L + C - 1, scattered over a pool whose
    every byte is random and finite; qkv rows [B * C, 3HD]."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    B = len(lens)
    need = [int(L - T0 + C - 1) // 32 + 1 for L in lens]
    npages = sum(need) + 3
    pool = _rand((npages, NLAYER, 2, H, 32, D), g, kv)
    width = max(need) + 2
    table = np.zeros((B, width), dtype=np.int64)
    page_bytes = pool[0].numel() * pool.element_size()
    perm = rng.permutation(npages)
    k = 0
    for b in range(B):
        for c in range(need[b]):
            table[b, c] = pool.data_ptr() + int(perm[k]) * page_bytes
            k += 1
    qkv = torch.randn((B * C, 3 * H * D), generator=g, device="cuda").half()
    kp, vp = _rand((H, max(T0, 1), D), g, kv), _rand((H, max(T0, 1), D), g, kv)
    return dict(B=B, C=C, T0=T0, kv=kv, lens_np=lens, pool=pool, table=torch.from_numpy(table).cuda(), qkv=qkv,
                kp=kp, vp=vp, fmt=_lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16)


def _prefix_args(c):
    T0 = c["T0"]
    return (c["kp"].data_ptr() if T0 else None, c["vp"].data_ptr() if T0 else None, c["kp"].stride(0) if T0 else 0, T0)


def _run_chunk(c, counts, table=None, window=0, C=None, expect=0):
    B, C = c["B"], c["C"] if C is None else C
    tab = c["table"] if table is None else table
    out = torch.full((B * max(C, 1), H * D), SENTINEL, device="cuda").half()
    lens = torch.from_numpy(c["lens_np"].astype(np.int32)).cuda()
    cnt = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
    rc = _lib.lib().ns_decode_attention_paged_chunk(
        c["qkv"].data_ptr(), c["qkv"].stride(0), tab.data_ptr(), tab.stride(0), tab.shape[1], LAYER * 2 * H * 32 * D,
        *_prefix_args(c), B, H, D, lens.data_ptr(), window, c["fmt"], C, cnt.data_ptr(), out.data_ptr(),
        out.stride(0), D ** -0.5, _stream_handle())
    assert rc == expect
    torch.cuda.synchronize()
    assert np.array_equal(lens.cpu().numpy(), c["lens_np"])  # d_lens is not advanced
    return out


def _run_one_by_one(c, counts, table=None):
    """The reference: the one-token kernel once per query index, streams past their count skipped (``d_stop``)."""
    B, C = c["B"], c["C"]
    tab = c["table"] if table is None else table
    out = torch.full((B, C, H * D), SENTINEL, device="cuda").half()
    counts = np.asarray(counts, dtype=np.int64)
    q3 = c["qkv"].view(B, C, -1)
    for i in range(int(counts.max(initial=0))):
        qkv = q3[:, i].contiguous()
        o = out[:, i].contiguous()
        lens = torch.from_numpy((c["lens_np"] + i).astype(np.int32)).cuda()
        stop = torch.from_numpy(np.where(counts > i, I32MAX, 0).astype(np.int32)).cuda()
        rc = _lib.lib().ns_decode_attention_paged(
            qkv.data_ptr(), qkv.stride(0), tab.data_ptr(), tab.stride(0), tab.shape[1], LAYER * 2 * H * 32 * D,
            *_prefix_args(c), B, H, D, lens.data_ptr(), 0, c["fmt"], None, 0, stop.data_ptr(), o.data_ptr(),
            o.stride(0), D ** -0.5, _stream_handle())
        assert rc == 0
        out[:, i] = o
    torch.cuda.synchronize()
    return out.view(B * C, H * D)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _compare(c, counts, table=None):
    pool0 = c["pool"].clone()
    ref = _run_one_by_one(c, counts, table)
    pool_ref = c["pool"].clone()
    c["pool"].copy_(pool0)
    out = _run_chunk(c, counts, table)
    assert _same_bits(out, ref)
    assert _same_bits(c["pool"], pool_ref)
    counts = np.asarray(counts)
    o3 = out.view(c["B"], c["C"], -1)
    for b in range(c["B"]):  # rows i >= n_b keep the sentinel; rows i < n_b were written
        assert (o3[b, counts[b]:] == SENTINEL).all(), b
        assert torch.isfinite(o3[b, : counts[b]].float()).all(), b
    c["pool"].copy_(pool0)
    return out, pool0, pool_ref


@functools.lru_cache(maxsize=4)
def _case(kv, C, T0):
    """Different lengths in one launch: a stream with no own rows (L = T0; L = 0 when T0 = 0), one whose chunk
    crosses the first page boundary, one short of the first split threshold, mid-page lengths."""
    lens = [T0, T0 + 30, 254, T0 + 77, T0 + 32, 300]
    return _build(kv, C, T0, lens, seed=100 * C + T0 + (1 if kv == "fp8" else 0))


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0", [0, 40])
@pytest.mark.parametrize("C", [1, 2, 5, 8, 16])
def test_chunk_equals_one_token_kernel_called_per_query(kv, T0, C):
    c = _case(kv, C, T0)
    _compare(c, [C] * c["B"])


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0", [0, 40])
def test_chunk_crosses_page_boundary_and_every_split_threshold(kv, T0):
    """C = 5 from L = 30 (page boundary at 32), 254, 510 and 1,022 (att_split 1->2, 2->4, 4->8 inside the chunk),
    L = T0 and, with T0 = 0, L = 0."""
    c = _build(kv, 5, T0, [max(30, T0), 254, 510, 1022, T0], seed=555 + T0)
    _compare(c, [5] * 5)


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0", [0, 40])
@pytest.mark.parametrize("C", [5, 16])
def test_counts_leave_later_rows_and_pages_alone(kv, T0, C):
    """Counts {0, 1, C - 1, C} in one launch (and a count above C, clamped): output rows i >= n_b keep the sentinel
    and no page byte past row L + n_b - 1 changes -- the pool equals the one-token reference's, which appended
    exactly n_b rows, byte for byte."""
    c = _case(kv, C, T0)
    counts = [0, 1, C - 1, C, 1, C - 1]
    out, pool0, pool_ref = _compare(c, counts)
    lens, tab = c["lens_np"], c["table"].cpu().numpy()
    page_bytes = pool0[0].numel() * pool0.element_size()
    changed = (pool_ref.view(torch.uint8) != pool0.view(torch.uint8)).view(pool0.shape[0], -1).any(dim=1).cpu().numpy()
    pg0 = int((tab[0, 0] - c["pool"].data_ptr()) // page_bytes)
    assert not changed[pg0]  # n_b = 0: the stream's page is untouched
    assert changed.sum() <= sum(2 for n in counts if n)  # at most two pages per running stream
    over = list(counts)
    over[3] = C + 9  # clamped to C
    ref = _run_one_by_one(c, counts)
    c["pool"].copy_(pool0)
    assert _same_bits(_run_chunk(c, over), ref)
    assert _same_bits(c["pool"], pool_ref)
    c["pool"].copy_(pool0)
    assert lens[0] == T0


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("hole", ["first", "second"])
def test_missing_page_poisons_the_stream_only(kv, hole):
    """A zeroed table entry for a stream's new rows: NaN in its n_b rows, no page byte of the pool changed by it;
    the other streams' rows and pages are those of the launch without the hole."""
    T0, C = 40, 5
    c = _case(kv, C, T0)
    counts = [C, C, C, 3, C, C]
    bad = 1  # L = T0 + 30: rows 30 .. 34 lie in chunks 0 and 1
    good, pool0, pool_good = _compare(c, counts)
    tab = c["table"].clone()
    tab[bad, 0 if hole == "first" else 1] = 0
    out = _run_chunk(c, counts, table=tab).view(c["B"], C, -1)
    g3 = good.view(c["B"], C, -1)
    assert torch.isnan(out[bad]).all()
    for b in range(c["B"]):
        if b != bad:
            assert _same_bits(out[b], g3[b]), b
    # the pool: the good launch's, except that the poisoned stream's pages are as they were
    page_bytes = pool0[0].numel() * pool0.element_size()
    expect = pool_good.clone()
    for e in c["table"][bad].cpu().numpy():
        if e:
            pg = int((e - c["pool"].data_ptr()) // page_bytes)
            expect[pg] = pool0[pg]
    assert _same_bits(c["pool"], expect)
    c["pool"].copy_(pool0)


def test_chunk_beyond_the_table_poisons():
    """New rows at a chunk >= max_chunks: NaN rows, nothing read past the table, nothing written."""
    c = _build("fp16", 5, 0, [30, 10], seed=77)
    pool0 = c["pool"].clone()
    tab = c["table"][:, :1].contiguous()  # max_chunks = 1: stream 0's rows 32 .. 34 have no entry
    out = _run_chunk(c, [5, 5], table=tab).view(2, 5, -1)
    assert torch.isnan(out[0]).all() and torch.isfinite(out[1].float()).all()
    page_bytes = pool0[0].numel() * pool0.element_size()
    pg = int((int(c["table"][0, 0]) - c["pool"].data_ptr()) // page_bytes)
    assert _same_bits(c["pool"][pg], pool0[pg])


def test_window_and_chunk_limits_are_rejected():
    c = _case("fp16", 5, 0)
    pool0 = c["pool"].clone()
    out = _run_chunk(c, [5] * c["B"], window=1, expect=_lib.NS_ERR_UNSUPPORTED)
    assert (out == SENTINEL).all()
    for C in (0, 17):
        out = _run_chunk(c, [1] * c["B"], C=C, expect=_lib.NS_ERR_CONFIG)
        assert (out == SENTINEL).all()
    assert _same_bits(c["pool"], pool0)
