"""GPU: the short-key path of the paged decode attention (``paged_attn_kernel<F, 8>``, ``csrc/nsg_attn.hip``).

Batches above the 1,024-pair threshold of the 8-pairs-per-workgroup form whose every key count is at most 256 and
whose context covers the first 32-row chunk (T0 >= 32, no window cutting it) take the short path: context chunk and
q requested at kernel entry, only rows below L0 loaded, wave w serving slot w.  It must give the SAME BITS as the
lockstep kernel (``ns_decode_attention_ex``) on every stream alone -- outputs and the appended K/V row -- and so must
the launches that fall back to the general path (T0 < 32, a cutting window, a workgroup mixing split and unsplit
pairs).  Every stream of every case is compared, none sampled.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from test_gpu_slots import D, H, _q8, _run_dense_one, _run_paged  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = [86, 90, 97, 200]  # > 1,024 / 12 pairs; no multiple of 8 or 16


def _lens(B, T0, rng, long_streams=0):
    special = [T0, T0 + 1, T0 + 30, T0 + 31, T0 + 32, T0 + 33, T0 + 63, T0 + 64, 254, 255]
    lens = np.concatenate([np.array(special * 2), rng.integers(T0, 256, size=B - 2 * len(special))])
    lens = rng.permutation(lens)
    if long_streams:  # key counts 257-301: split over two waves, their workgroups leave the short path
        lens[rng.choice(B, size=long_streams, replace=False)] = rng.integers(256, 301, size=long_streams)
    return lens


def _build(B, T0, kv, lens, seed, n_layer=2, layer=1):
    """``test_gpu_slots._paged_case`` with given per-stream lengths: dense rows [B, H, rows, D] and the same rows
    scattered over a page pool in random order."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    rows = int(lens.max() - T0 + 1)
    nch = (rows + 31) // 32
    qkv = torch.randn((B, 3 * H * D), generator=g, device="cuda").half()
    dk = torch.randn((B, H, nch * 32, D), generator=g, device="cuda").half()
    dv = torch.randn((B, H, nch * 32, D), generator=g, device="cuda").half()
    kp = torch.randn((H, max(T0, 1), D), generator=g, device="cuda").half()
    vp = torch.randn((H, max(T0, 1), D), generator=g, device="cuda").half()
    if kv == "fp8":
        dk, dv, kp, vp = _q8(dk), _q8(dv), _q8(kp), _q8(vp)
    need = [(int(L) - T0) // 32 + 1 for L in lens]  # pages through the new token's row
    npages = sum(need) + 3
    pool = torch.zeros((npages, n_layer, 2, H, 32, D), dtype=dk.dtype, device="cuda")
    perm = rng.permutation(npages)
    table = np.zeros((B, nch + 2), dtype=np.int64)
    page_of = np.full((B, nch + 2), -1, dtype=np.int64)
    page_bytes = pool[0].numel() * pool.element_size()
    k = 0
    for b in range(B):
        for c in range(need[b]):
            pg = int(perm[k])
            k += 1
            pool[pg, layer, 0] = dk[b, :, 32 * c: 32 * c + 32]
            pool[pg, layer, 1] = dv[b, :, 32 * c: 32 * c + 32]
            table[b, c] = pool.data_ptr() + pg * page_bytes
            page_of[b, c] = pg
    return dict(qkv=qkv, dk=dk, dv=dv, kp=kp, vp=vp, pool=pool, table=torch.from_numpy(table).cuda(),
                lens=torch.from_numpy(lens.astype(np.int32)).cuda(), lens_np=lens, nch=nch, layer=layer, T0=T0,
                page_of=page_of, fmt=_lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16)


@functools.lru_cache(maxsize=2)
def _case(kv, B, T0, window, long_streams=0):
    """One case, its untouched pool, and the lockstep kernel's result on every stream alone (computed once, shared,
    never modified)."""
    seed = 1000 * B + 10 * T0 + window + (1 if kv == "fp8" else 0) + 7 * long_streams
    lens = _lens(B, T0, np.random.default_rng(seed), long_streams)
    c = _build(B, T0, kv, lens, seed)
    refs = [_run_dense_one(c, b, window) for b in range(B)]
    return c, c["pool"].clone(), refs


def _check_all(c, refs, out, streams=None):
    T0, lay, pool = c["T0"], c["layer"], c["pool"]
    for b in range(len(refs)) if streams is None else streams:
        ref, kref, vref = refs[b]
        assert torch.equal(out[b], ref), b
        r = int(c["lens_np"][b]) - T0  # the appended row landed in the stream's page
        pg = int(c["page_of"][b, r // 32])
        assert torch.equal(pool[pg, lay, 0, :, r % 32], kref[:, r]), b
        assert torch.equal(pool[pg, lay, 1, :, r % 32], vref[:, r]), b
    assert not pool[:, 1 - lay].any()  # the other layer's blocks untouched


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("T0,window", [(32, 0), (40, 0),  # the short path
                                       (0, 0), (7, 0), (32, 40)])  # the general path: no whole context chunk, cut
def test_short_keys_equal_lockstep_kernel_on_every_stream(kv, B, T0, window):
    c, pool0, refs = _case(kv, B, T0, window)
    c["pool"].copy_(pool0)
    out = _run_paged(c, B, window)
    assert torch.isfinite(out.float()).all()
    _check_all(c, refs, out)


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_workgroups_mixing_split_and_unsplit_pairs_leave_the_short_path(kv):
    B = 97
    c, pool0, refs = _case(kv, B, 32, 0, long_streams=5)
    assert (c["lens_np"] >= 256).sum() == 5 and (c["lens_np"] < 256).sum() == B - 5
    c["pool"].copy_(pool0)
    out = _run_paged(c, B)
    _check_all(c, refs, out)


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0", [32, 40])
def test_short_keys_skips_and_poison(kv, T0):
    """Every fifth stream done and one stream without its new-token page: skipped rows untouched and nothing
    written for them, the poisoned stream NaN with nothing written, every other stream's bits as unskipped."""
    B = 90
    c, pool0, refs = _case(kv, B, T0, 0)
    flags = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    flags[::5, 3] = 1
    bad = 12  # not a multiple of 5
    tab = c["table"].clone()
    r = int(c["lens_np"][bad]) - T0
    tab[bad, r // 32] = 0
    c["pool"].copy_(pool0)
    out = _run_paged(c, B, done=flags[:, 3], table=tab)
    run = [b for b in range(B) if b % 5 and b != bad]
    assert (out[::5] == 7.0).all()
    assert torch.isnan(out[bad]).all()
    _check_all(c, refs, out, streams=run)
    for b in list(range(0, B, 5)) + [bad]:  # nothing written: the stream's pages are as built
        for pg in c["page_of"][b]:
            if pg >= 0:
                assert torch.equal(c["pool"][pg], pool0[pg]), b


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
@pytest.mark.parametrize("T0", [32, 40])
def test_rows_past_the_new_token_are_never_read(kv, T0):
    """NaN in every row past L0 of each stream's last page (K and V): those rows are never loaded, so the outputs
    are finite and unchanged."""
    B = 86
    c, pool0, refs = _case(kv, B, T0, 0)
    c["pool"].copy_(pool0)
    nan = 0x7F if kv == "fp8" else float("nan")  # e4m3fn NaN byte
    for b in range(B):
        r = int(c["lens_np"][b]) - T0
        pg = int(c["page_of"][b, r // 32])
        c["pool"][pg, c["layer"], :, :, r % 32 + 1:] = nan
    out = _run_paged(c, B)
    assert torch.isfinite(out.float()).all()
    for b in range(B):
        assert torch.equal(out[b], refs[b][0]), b
        r = int(c["lens_np"][b]) - T0
        pg = int(c["page_of"][b, r // 32])
        assert torch.equal(c["pool"][pg, c["layer"], 0, :, r % 32], refs[b][1][:, r]), b
        assert torch.equal(c["pool"][pg, c["layer"], 1, :, r % 32], refs[b][2][:, r]), b
