"""GPU: the ragged prefill attention CONTINUED from KV pages (``ns_seq_attention_ragged_past``).

A sequence whose first P rows (a multiple of 64) another launch already stored in pages is run from row P on: key
blocks below P / 64 come from the pages, the others from the packed rows, in the one block body.  fp16 pages hold bit
copies of the qkv values, so every comparison below is bit equality against ``ns_seq_attention_ragged`` over the whole
sequence: the output rows P.., the stored rows, and every other byte of the page pool (prefix pages untouched, the
rest still the poison).  The pool and the outputs start as poison, and every address a launch is given is valid
memory: the guard checks hand the kernel bad COUNTS and zero entries, never a bad address."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import ragged_blocks  # noqa: E402

pytestmark = pytest.mark.gpu

H, D = 2, 64
C = H * D
N_LAYER, LAYER = 2, 1
LAYER_OFF = LAYER * 2 * H * 32 * D
# (T, P): the whole length and the rows already in pages.  65 / 129: one new row; 100, 200: a ragged tail; 192: new
# rows that are one whole block; then a sequence with no past and an unrelated one
CASES = [(65, 64), (100, 64), (129, 128), (200, 128), (192, 128), (70, 0), (45, 0)]
POISON = 0xA5


def _out(rows):
    o = torch.empty((rows, C), device="cuda", dtype=torch.float16)
    o.view(torch.uint8).fill_(POISON)
    return o


def _whole(qkv, lens, table, seq_slot, out=None):
    seq_start, blocks = ragged_blocks(lens)
    R = int(seq_start[-1])
    out = _out(R) if out is None else out
    ds, db = torch.from_numpy(seq_start).cuda(), torch.from_numpy(blocks).cuda()
    rc = _lib.lib().ns_seq_attention_ragged(
        qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), ds.data_ptr(), len(lens), R, db.data_ptr(),
        blocks.shape[0], H, D, D ** -0.5, table.data_ptr(), table.stride(0), table.shape[1], seq_slot.data_ptr(),
        table.shape[0], LAYER_OFF, _lib.NS_KV_FP16, _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _past_rc(qkv, new_lens, past, table, seq_slot, out, max_chunks=None, **kw):
    seq_start, blocks = ragged_blocks(new_lens)
    R = int(seq_start[-1])
    ds, db = torch.from_numpy(seq_start).cuda(), torch.from_numpy(blocks).cuda()
    dp = torch.from_numpy(np.asarray(past, dtype=np.int32)).cuda()
    a = dict(tab=table.data_ptr(), dpast=dp.data_ptr(), D=D, fmt=_lib.NS_KV_FP16)
    a.update(kw)
    rc = _lib.lib().ns_seq_attention_ragged_past(
        qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), ds.data_ptr(), a["dpast"], len(new_lens), R,
        db.data_ptr(), blocks.shape[0], H, a["D"], D ** -0.5, a["tab"], table.stride(0),
        table.shape[1] if max_chunks is None else max_chunks, seq_slot.data_ptr(), table.shape[0], LAYER_OFF,
        a["fmt"], _stream_handle())
    torch.cuda.synchronize()
    return rc, seq_start


def _past(qkv, new_lens, past, table, seq_slot, max_chunks=None):
    out = _out(int(sum(new_lens)))
    rc, seq_start = _past_rc(qkv, new_lens, past, table, seq_slot, out, max_chunks)
    assert rc == 0
    return out, seq_start


class World:
    """The CASES sequences, each with a FIRST slot (its whole length prefilled at once) and a SECOND slot whose table
    row starts with the first slot's P / 32 pages and continues with pages of its own; ``after_whole`` is the pool
    after the whole prefill, ``whole`` its output (computed once, never changed)."""

    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(31)
        rng = np.random.default_rng(31)
        self.T = [t for t, _ in CASES]
        self.P = [p for _, p in CASES]
        n = len(CASES)
        self.start = np.concatenate([[0], np.cumsum(self.T)])
        self.qkv = torch.randn((int(self.start[-1]), 3 * C), generator=g, device="cuda").half()
        need = [-(-t // 32) for t in self.T]
        width = max(need) + 1  # the entry after a sequence's last page stays 0
        npages = sum(need) + sum(nd - p // 32 for nd, p in zip(need, self.P)) + 3
        self.pool = torch.empty((npages, N_LAYER, 2, H, 32, D), dtype=torch.float16, device="cuda")
        self.pool.view(torch.uint8).fill_(POISON)
        self.page_bytes = self.pool[0].numel() * 2
        ids = iter(rng.permutation(npages).tolist())
        self.page = {}  # (slot kind, sequence, column) -> page index
        table = np.zeros((2 * n + 1, width), dtype=np.int64)
        self.first = rng.permutation(2 * n + 1)[: 2 * n]
        self.second = self.first[n:]
        self.first = self.first[:n]
        for s in range(n):
            for c in range(need[s]):
                self.page[(0, s, c)] = next(ids)
                table[self.first[s], c] = self.addr(self.page[(0, s, c)])
                own = c >= self.P[s] // 32
                self.page[(1, s, c)] = next(ids) if own else self.page[(0, s, c)]
                table[self.second[s], c] = self.addr(self.page[(1, s, c)])
        self.need, self.table_host = need, table
        self.table = torch.from_numpy(table).cuda()
        self.d_first = torch.from_numpy(self.first.astype(np.int32)).cuda()
        self.d_second = torch.from_numpy(self.second.astype(np.int32)).cuda()
        self.whole = _whole(self.qkv, self.T, self.table, self.d_first)
        self.after_whole = self.pool.clone()
        blank = torch.empty_like(self.pool)
        blank.view(torch.uint8).fill_(POISON)
        assert torch.equal(self.after_whole.view(torch.uint8), self.expect(blank, 0, [0] * n).view(torch.uint8))
        # the new rows only, packed
        self.new_lens = [t - p for t, p in zip(self.T, self.P)]
        self.new_qkv = torch.cat([self.qkv[self.start[s] + self.P[s]: self.start[s + 1]] for s in range(n)])
        self.new_start = np.concatenate([[0], np.cumsum(self.new_lens)])

    def addr(self, page):
        return self.pool.data_ptr() + page * self.page_bytes

    def expect(self, base, kind, from_row, only=None):
        """``base`` with rows ``from_row[s]`` .. T-1 of every sequence (``only``: of these) in its pages of slot
        ``kind``."""
        want = base.clone()
        k = self.qkv[:, C:2 * C].contiguous().view(-1, H, D)
        v = self.qkv[:, 2 * C:].contiguous().view(-1, H, D)
        for s in (range(len(self.T)) if only is None else only):
            a = int(self.start[s])
            for c in range(from_row[s] // 32, self.need[s]):
                r0, r1 = 32 * c, min(32 * c + 32, self.T[s])
                want[self.page[(kind, s, c)], LAYER, 0, :, : r1 - r0] = k[a + r0:a + r1].transpose(0, 1)
                want[self.page[(kind, s, c)], LAYER, 1, :, : r1 - r0] = v[a + r0:a + r1].transpose(0, 1)
        return want

    def whole_rows(self, s):
        return self.whole[self.start[s] + self.P[s]: self.start[s + 1]]


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture()
def fresh(world):
    """The pool as the whole prefill left it (the tests below write the second slots' pages)."""
    world.pool.copy_(world.after_whole)
    return world


def test_continued_rows_and_pages_equal_the_whole_prefill_in_one_launch(fresh):
    w = fresh
    out, st = _past(w.new_qkv, w.new_lens, w.P, w.table, w.d_second)
    for s, (T, P) in enumerate(CASES):
        assert torch.equal(out[st[s]: st[s + 1]], w.whole_rows(s)), (T, P)
    # the second slots' own pages hold rows P.. exactly as the first slots' pages do; the prefix pages and every
    # other byte (rows past a sequence's end, layer 0, spare pages) are as they were
    want = w.expect(w.after_whole, 1, w.P)
    assert torch.equal(w.pool.view(torch.uint8), want.view(torch.uint8))
    for s, (T, P) in enumerate(CASES):
        for c in range(P // 32, w.need[s]):
            assert torch.equal(w.pool[w.page[(1, s, c)], LAYER], w.pool[w.page[(0, s, c)], LAYER]), (T, P, c)


@pytest.mark.parametrize("s", range(len(CASES)))
def test_a_sequence_does_not_depend_on_what_is_packed_around_it(fresh, s):
    """Every other sequence's new rows NaN and every other sequence's pages NaN: a read outside the sequence's own
    rows and its own table row would reach its output (a masked key contributes 0 x NaN = NaN)."""
    w = fresh
    T, P = CASES[s]
    qkv = torch.full_like(w.new_qkv, float("nan"))
    a, b = int(w.new_start[s]), int(w.new_start[s + 1])
    qkv[a:b] = w.new_qkv[a:b]
    for (kind, t, c), page in w.page.items():
        if t != s:
            w.pool[page] = float("nan")
    out, st = _past(qkv, w.new_lens, w.P, w.table, w.d_second)
    assert torch.equal(out[a:b], w.whole_rows(s)), (T, P)
    for c in range(w.need[s]):
        assert torch.equal(w.pool[w.page[(1, s, c)]], w.expect(w.after_whole, 1, w.P, only=[s])[w.page[(1, s, c)]])
    # alone in a launch of its own: the same bits
    w.pool.copy_(w.after_whole)
    alone, _ = _past(w.new_qkv[a:b].contiguous(), [T - P], [P], w.table, w.d_second[s:s + 1].contiguous())
    assert torch.equal(alone, w.whole_rows(s)), (T, P)
    assert torch.equal(w.pool.view(torch.uint8), w.expect(w.after_whole, 1, w.P, only=[s]).view(torch.uint8))


def test_all_zero_past_is_the_ragged_form_bit_for_bit(world):
    w = world
    w.pool.view(torch.uint8).fill_(POISON)
    out, _ = _past(w.qkv, w.T, [0] * len(w.T), w.table, w.d_first)
    assert torch.equal(out, w.whole)
    assert torch.equal(w.pool.view(torch.uint8), w.after_whole.view(torch.uint8))


def test_entry_point_refusals(fresh):
    w = fresh
    before = w.pool.clone()
    out = _out(int(sum(w.new_lens)))
    args = (w.new_qkv, w.new_lens, w.P, w.table, w.d_second, out)
    assert _past_rc(*args, fmt=_lib.NS_KV_FP8)[0] == _lib.NS_ERR_UNSUPPORTED
    assert _past_rc(*args, tab=None)[0] == _lib.NS_ERR_CONFIG
    assert _past_rc(*args, dpast=None)[0] == _lib.NS_ERR_CONFIG
    assert _past_rc(*args, D=32)[0] == _lib.NS_ERR_CONFIG
    assert _past_rc(*args, fmt=2)[0] == _lib.NS_ERR_CONFIG
    assert (out.view(torch.uint8) == POISON).all() and torch.equal(w.pool.view(torch.uint8), before.view(torch.uint8))


def test_device_guards_retire_a_bad_sequence_and_serve_the_good_one(fresh):
    """One launch: sequence 1 (T 100, P 64) as it is; sequence 0 with ``past`` 32; sequence 3 with its second past
    table entry zeroed; sequence 4 (P 128 = 4 pages) under ``max_chunks`` 3... every table entry that stays is a
    valid page, and the table is wider than ``max_chunks``: the launch is given no address it could fault on."""
    w = fresh
    use = [1, 0, 3, 4]
    past = [64, 32, 128, 128]
    tab = w.table_host.copy()
    tab[w.second[3], 1] = 0
    # max_chunks 3: sequence 4's past pages 0..3 reach beyond it; sequence 3 would be refused for that too, so it
    # runs in a launch of its own below with the full width
    qkv = torch.cat([w.new_qkv[w.new_start[s]: w.new_start[s + 1]] for s in use])
    lens = [w.new_lens[s] for s in use]
    slot = torch.from_numpy(w.second[use].astype(np.int32)).cuda()
    out, st = _past(qkv, lens, past, torch.from_numpy(tab).cuda(), slot, max_chunks=3)
    assert torch.equal(out[st[0]: st[1]], w.whole_rows(1))
    assert (out[st[1]:].view(torch.uint8) == POISON).all()
    # the good sequence's rows below chunk 3 are stored (rows 64..95; 96..99 lie in chunk 3 >= max_chunks)
    want = w.after_whole.clone()
    want[w.page[(1, 1, 2)], LAYER] = w.expect(w.after_whole, 1, w.P, only=[1])[w.page[(1, 1, 2)], LAYER]
    assert torch.equal(w.pool.view(torch.uint8), want.view(torch.uint8))
    # the zero entry and the odd past at the table's full width, next to the good sequence
    w.pool.copy_(w.after_whole)
    out, st = _past(qkv[: st[3]].contiguous(), lens[:3], past[:3], torch.from_numpy(tab).cuda(),
                    slot[:3].contiguous())
    assert torch.equal(out[st[0]: st[1]], w.whole_rows(1))
    assert (out[st[1]:].view(torch.uint8) == POISON).all()
    assert torch.equal(w.pool.view(torch.uint8), w.expect(w.after_whole, 1, w.P, only=[1]).view(torch.uint8))
    # a negative past
    out, st = _past(qkv[: st[2]].contiguous(), lens[:2], [64, -64], torch.from_numpy(tab).cuda(),
                    slot[:2].contiguous())
    assert torch.equal(out[st[0]: st[1]], w.whole_rows(1)) and (out[st[1]:].view(torch.uint8) == POISON).all()
