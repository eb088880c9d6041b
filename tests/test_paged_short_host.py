"""CPU: a restatement of the SHORT-KEY path of ``paged_attn_kernel<F, 8>`` (``csrc/nsg_attn.hip``): which rows it
loads per (iteration, slab, row group), from which context or page address, and which workgroup wave serves which
(stream, head) pair.

The short path is taken by a workgroup (8 streams of one head) when the context covers the first whole 32-row chunk
(T0 >= 32), no pair is split over waves (every key count <= 256) and no window cuts the first chunk (every pair's
keys start at position 0).  Wave w serves the pair of slot w.  It loads the context's rows 0..31 at kernel entry,
the stream's page addresses 0..cN (cN = the new token's chunk) in one load, then per 32-row iteration only the rows
below L0: row L0 is the new token (from the qkv row), rows past it are fed zeros and masked.  An address computed for
an unmapped chunk would fault the GPU; a row fed to the arithmetic out of order would change the bits.  This test
walks the same arithmetic over T0, every L0 and the batch tails and fails on either.  (Two pairs per wave slot is
not built: the placement checked is the one the kernel has, one pair per wave.)"""

import pytest

H = 12
ROWS1 = 256


def att_split(lk):
    return 1 if lk <= ROWS1 else 2 if lk <= 2 * ROWS1 else 4 if lk <= 4 * ROWS1 else 8


def pair_state(T0, L0, window, skipped, max_chunks=64):
    """The setup's (status, s0, S) of a slot: status 0 none / skipped, 1 run, 2 poison."""
    if skipped:
        return 0, 0, 0
    jj = L0 - T0
    if not (jj >= 0 and (jj >> 5) < max_chunks):
        return 2, 0, 0
    lk = L0 + 1
    s0 = max(0, lk - window) if window > 0 else 0
    return 1, s0, att_split(lk - s0)


def takes_short_path(T0, states):
    """Uniform over the workgroup: the context holds the first chunk, no pair split, no first chunk cut."""
    return T0 >= 32 and not any(S > 1 for _, _, S in states) and not any(s0 != 0 for _, s0, _ in states)


def short_path_rows(T0, L0):
    """The loads a wave issues for one pair and the rows its arithmetic sees, in order.

    Returns (loads, seen): loads = [("ctx", row) | ("page", chunk, row_in_page)], seen = [(position, source)] of the
    rows that reach the softmax as valid, source "ctx" / "page" / "new"."""
    assert T0 >= 32 and T0 <= L0 <= ROWS1 - 1
    cN = (L0 - T0) >> 5
    assert cN <= 7  # the page addresses live one per lane in lanes 0..7
    table_lanes = [lane for lane in range(64) if lane <= cN]  # lane i loads trow[i]
    loads, seen = [], []
    for r in range(32):  # entry: iteration 0, the context's first chunk, every row valid
        loads.append(("ctx", r))
        seen.append((r, "ctx"))
    j0 = 32
    while j0 <= L0:
        jj0 = j0 - T0
        ca = max(jj0, 0) >> 5
        assert ca + 1 <= 7  # readlane index of pb
        interior = jj0 >= 0 and j0 + 32 <= L0
        for r in range(32):  # r = 8 * u + g (fp16) or 16 * u + g (fp8): the same 32 rows either way
            row = j0 + r
            if interior:
                jj = jj0 + r
                chunk = ca if (jj >> 5) == ca else ca + 1
                loads.append(("page", chunk, jj & 31))
                assert chunk == jj >> 5 and chunk in table_lanes
                seen.append((row, "page"))
                continue
            if row < T0:
                loads.append(("ctx", row))
                seen.append((row, "ctx"))
            elif row < L0:
                jj = row - T0
                chunk = ca if (jj >> 5) == ca else ca + 1
                assert chunk == jj >> 5
                loads.append(("page", chunk, jj & 31))
                seen.append((row, "page"))
            elif row == L0:
                seen.append((row, "new"))  # from the qkv row; appended to page cN at row (L0 - T0) & 31
            # rows past L0: no load, zeros, masked
        j0 += 32
    return loads, seen, cN


@pytest.mark.parametrize("T0", [32, 40, 64])
def test_short_path_loads_and_row_order(T0):
    for L0 in range(T0, 301):
        status, s0, S = pair_state(T0, L0, 0, False)
        assert status == 1 and s0 == 0
        if L0 + 1 > ROWS1:  # a split pair: the workgroup leaves the short path
            assert S > 1 and not takes_short_path(T0, [(status, s0, S)])
            continue
        assert takes_short_path(T0, [(status, s0, S)])
        loads, seen, cN = short_path_rows(T0, L0)
        mapped = set(range(((L0 - T0) >> 5) + 1))  # host invariant: pages through the new token's chunk
        assert cN in mapped
        for ld in loads:
            if ld[0] == "ctx":
                assert 0 <= ld[1] < T0, (T0, L0, ld)
            else:
                assert ld[1] in mapped and 0 <= ld[2] < 32, (T0, L0, ld)
                assert T0 + 32 * ld[1] + ld[2] < L0, (T0, L0, ld)  # a cached row: never the new token's or a later one
        assert [p for p, _ in seen] == list(range(L0 + 1)), (T0, L0)
        for p, src in seen:
            assert src == ("ctx" if p < T0 else "new" if p == L0 else "page"), (T0, L0, p, src)
        # no load is issued twice and none is wasted: one per cached row
        assert len(loads) == len(set(loads)) == L0


@pytest.mark.parametrize("T0,window,short", [(32, 0, True), (40, 0, True), (32, 40, False), (0, 0, False),
                                             (7, 0, False), (31, 0, False)])
def test_short_path_choice(T0, window, short):
    lens = [T0, T0 + 1, T0 + 5, T0 + 7, T0 + 30, T0 + 63, 200, 255]
    states = [pair_state(T0, L, window, False) for L in lens]
    assert takes_short_path(T0, states) == short
    # one split pair (S = 2) takes the whole workgroup off the short path
    assert not takes_short_path(T0, states[:7] + [pair_state(T0, 256, window, False)])
    # a window that cuts no pair's first chunk keeps it (keys still start at position 0)
    if T0 >= 32:
        assert takes_short_path(T0, [pair_state(T0, L, 256, False) for L in lens])
        assert not takes_short_path(T0, [pair_state(T0, L, 255, False) for L in lens])


@pytest.mark.parametrize("B", [86, 90, 97, 200, 128, 1])
def test_every_pair_served_once_and_skips_shift_nothing(B):
    grid = H * ((B + 7) // 8)
    for skipped in (set(), set(range(0, B, 5)), set(range(B))):
        served = {}
        for gidx in range(grid):
            h = gidx % H
            for wave in range(8):  # wave w <-> slot w, whatever the other slots' state
                b = (gidx // H) * 8 + wave
                entry_b = min(b, B - 1)  # the entry q load's stream index: always inside the batch
                assert 0 <= entry_b < B
                if b >= B:
                    continue  # no pair: the wave retires
                if b in skipped:
                    continue  # status 0: the wave retires, nothing read or written
                assert (b, h) not in served
                served[(b, h)] = (gidx, wave)
        assert set(served) == {(b, h) for b in range(B) if b not in skipped for h in range(H)}
        if not skipped:
            base = served
        else:  # the pairs that run are served by the same workgroup and wave as in the unskipped launch
            assert all(base[k] == v for k, v in served.items())
