"""CPU: the staging map, fragment reads and wait counts of gemm_ph96 (csrc/nsg_lm.hip), restated and checked.

The kernel's correctness rests on index arithmetic that a GPU run checks only through the result: which LDS-DMA
instruction of which wave fills which 16-byte chunk, where a fragment read finds its (row, k), and how many copies
each counted vmcnt leaves in flight.  This file restates that arithmetic and checks:

* every 16-byte chunk of a staged K-tile (224 rows x 8 chunks) is written exactly once, by the ragged four-
  instruction map (instruction 3 exists in waves 0..3 only), with the logical chunk the swizzle promises;
* every fragment read hits the physical chunk that holds its (row, k), and the eight waves' sub-tiles cover the
  96 x 128 tile exactly once;
* for 1 .. 8 K-tiles, every wait leaves exactly the K-tiles after the next one in flight (at most two), a K-tile
  is read only in a slot after the barrier that follows BOTH groups' waits for it, and a ring buffer is refilled
  only in a slot after the barrier that follows both groups' last reads of it.
"""

import pytest

BN, BM, NST, WAVES = 96, 128, 4, 8
ROWS = BN + BM
FN, FM = 3, 2


def swz(row):
    return (row >> 1) & 7


def instructions(wave):
    """LDS-DMA instructions of a wave per K-tile: 0..2 everywhere, 3 in group 0 (waves 0..3) only."""
    return range(4 if wave < 4 else 3)


def staged_chunks(wave, i):
    """(LDS row, physical chunk, logical chunk copied there) for the 64 lanes of instruction i of a wave."""
    out = []
    for lane in range(64):
        piece = 8 * i + wave
        byte = piece * 1024 + lane * 16          # wave-uniform base + lane * 16
        row, phys = byte // 128, (byte % 128) // 16
        logical = (lane & 7) ^ (((wave & 1) * 4 + (lane >> 4)) & 7)  # the kernel's per-wave source chunk
        out.append((row, phys, logical))
    return out


def test_every_chunk_is_staged_once_with_the_swizzled_content():
    seen = {}
    for wave in range(WAVES):
        for i in instructions(wave):
            for row, phys, logical in staged_chunks(wave, i):
                assert (row, phys) not in seen, (wave, i, row, phys)
                seen[(row, phys)] = logical
    assert len(seen) == ROWS * 8 and set(seen) == {(r, c) for r in range(ROWS) for c in range(8)}
    for (row, phys), logical in seen.items():
        assert logical == phys ^ swz(row), (row, phys)  # physical chunk p of row r holds logical chunk p ^ swz(r)


def test_pieces_do_not_straddle_the_operands():
    for wave in range(WAVES):
        for i in instructions(wave):
            rows = {r for r, _, _ in staged_chunks(wave, i)}
            assert len(rows) == 8 and (max(rows) < BN or min(rows) >= BN)
    assert sum(len(instructions(w)) for w in range(WAVES)) == ROWS // 8


def test_fragment_reads_hit_their_chunk_and_cover_the_tile():
    covered = {}
    for wave in range(WAVES):
        g, wn, wm = wave >> 2, (wave >> 1) & 1, wave & 1
        for lane in range(64):
            fr, fc = lane & 15, lane >> 4
            for kk in range(2):
                ch = kk * 4 + fc                 # logical chunk: k = 32 kk + 8 fc .. + 7
                for i in range(FN):
                    row = wn * FN * 16 + i * 16 + fr
                    assert 0 <= row < BN
                    assert ((ch ^ swz(row)) ^ swz(row)) == ch and 0 <= (ch ^ swz(row)) < 8
                for j in range(FM):
                    row = BN + g * 64 + wm * FM * 16 + j * 16 + fr
                    assert BN <= row < ROWS
                    assert 0 <= (ch ^ swz(row)) < 8
            # the outputs of this lane: weight row n = wn * 48 + 16 i + 4 fc + r, activation row m
            for i in range(FN):
                for j in range(FM):
                    for r in range(4):
                        n = wn * FN * 16 + i * 16 + 4 * fc + r
                        m = g * 64 + wm * FM * 16 + j * 16 + fr
                        assert (n, m) not in covered
                        covered[(n, m)] = wave
    assert len(covered) == BN * BM


def schedule(KT):
    """Replay one wave group's waits.  Returns per group: {tile: slot of the wait that retires it}, the in-flight
    tile sets after each wait, and the slots of reads and refills.  Slot of group g's L slot of K-tile t: 2 t + g
    (the prologue is slot -1; a barrier ends every slot)."""
    res = []
    for g in range(2):
        ni = 4 if g == 0 else 3
        queue, landed_at, flight_after, reads, fills = [], {}, {}, {}, {}

        def issue(tile, slot):
            queue.extend([tile] * ni)
            fills[tile] = slot

        def wait(tiles, slot):
            count = ni * min(tiles, 2) if tiles >= 1 else 0  # wait_tiles(): vmcnt(2 NI), vmcnt(NI) or vmcnt(0)
            while len(queue) > count:
                tile = queue.pop(0)
                if tile not in queue:  # its last copy: the K-tile has landed for this wave
                    landed_at[tile] = slot

        for s0 in range(NST - 1):
            if s0 < KT:
                issue(s0, -1)
        wait(min(KT - 1, 2), -1)
        flight_after[-1] = sorted(set(queue))
        for kt in range(KT):
            slot = 2 * kt + g
            reads[kt] = slot
            if kt + NST - 1 < KT:
                issue(kt + NST - 1, slot)
            if kt + 1 < KT:
                wait(min(KT - 2 - kt, 2), slot)
                flight_after[kt] = sorted(set(queue))
        assert not queue, "every copy is waited for before the epilogue's loads"
        res.append((landed_at, flight_after, reads, fills))
    return res


@pytest.mark.parametrize("KT", range(1, 9))
def test_wait_counts_leave_the_intended_tiles_in_flight(KT):
    groups = schedule(KT)
    for landed_at, flight_after, reads, fills in groups:
        assert flight_after[-1] == [t for t in (1, 2) if t < KT]
        for kt in range(KT - 1):
            # after the wait in K-tile kt's L slot: kt + 1 has landed, exactly kt + 2 and kt + 3 (if any) fly
            assert flight_after[kt] == [t for t in (kt + 2, kt + 3) if t < KT], (KT, kt)
            if kt + 2 < KT:
                assert flight_after[kt], "no drain to zero while later K-tiles exist"
        assert sorted(landed_at) == list(range(KT))
    for tile in range(KT):
        retired = max(grp[0][tile] for grp in groups)      # the later of the two groups' waits
        first_read = min(grp[2][tile] for grp in groups)
        assert first_read > retired, (KT, tile)             # a barrier ends slot `retired`
        if tile >= NST:
            last_read_prev = max(grp[2][tile - NST] for grp in groups)  # same ring buffer, the tile before
            first_fill = min(grp[3][tile] for grp in groups)
            assert first_fill > last_read_prev, (KT, tile)
