"""CPU: page ownership of shared contexts (``lm/kvpages.py``, library 0.30) and the admission estimate of the slot
schedulers (``lm/slots.py``).  Messages of one call that carry the same context hold one entry of the call's registry:
the entry owns the context's full pages and a master tail page, a holder's table row starts with the full pages and
continues with its own.  Every page goes back to the pool exactly once, whatever the order of releases; the device
side is covered by ``tests/test_gpu_context_share.py``."""

import itertools
from collections import deque

import numpy as np
import pytest
import torch

from neuralsteganography_amd.lm.kvpages import (PAGE_ROWS, KVPagePool, PagedKV, own_pages, shared_pages,
                                                   sharing_keys)
from neuralsteganography_amd.lm.slots import _admissible, _multiplicity


def _pool(seg_pages=8, budget_pages=None):
    holder = {}
    budget = None
    if budget_pages is not None:
        def budget():
            return (budget_pages - holder["pool"].total) * holder["pool"].page_bytes
    pool = KVPagePool(n_layer=2, n_head=2, head_dim=64, dtype=torch.float16, device="cpu", budget_bytes=budget,
                      seg_pages=seg_pages)
    holder["pool"] = pool
    return pool


A, B_, C = tuple(range(65)), tuple(range(100, 164)), tuple(range(200, 231))  # 65 (tail 1), 64 (no tail), 31 (no full)


def _admit(kv, slots, keys, ahead=17):
    slots = np.asarray(slots)
    tl = np.asarray([len(k) for k in keys])
    kv.reset(slots, lens=tl)
    assert kv.hold(slots, keys, tl).size == 0
    assert kv.ensure(slots, tl + ahead).size == 0


def _check_books(kv, pool):
    """Every page of the pool is free, an entry's, or in exactly one slot's own columns."""
    tab = kv.host
    assert (kv.table.numpy() == tab).all()
    own = [int(p) for s in range(kv.B) for p in tab[s, kv.nshared[s]: kv.nch[s]]]
    ent = [int(p) for e in kv.entries.values() for p in e.pages]
    free = pool._free[: pool.free_pages].tolist()
    everything = own + ent + free
    assert len(everything) == pool.total and len(set(everything)) == pool.total and 0 not in everything
    assert kv.in_use == len(own) + len(ent)
    for s in range(kv.B):
        e = kv.slot_entry[s]
        assert kv.nshared[s] == (e.full if e is not None else 0)
        if e is not None:
            assert tab[s, : e.full].tolist() == e.pages[: e.full].tolist()
        assert not tab[s, kv.nch[s]:].any()
    assert sorted(e.holders for e in kv.entries.values()) == sorted(
        sum(1 for x in kv.slot_entry if x is e) for e in kv.entries.values())


def test_holders_share_full_pages_and_own_their_tail_and_later_pages():
    pool = _pool()
    kv = PagedKV(pool, 6, 0, 2)
    slots = [4, 0, 2, 5, 1]
    _admit(kv, slots, [A, A, B_, B_, C])
    _check_books(kv, pool)
    # A: 2 full + master tail; B_: 2 full; C: 0 full + master tail
    assert {k: e.pages.size for k, e in kv.entries.items()} == {A: 3, B_: 2, C: 1}
    assert [shared_pages(len(k)) for k in (A, B_, C)] == [3, 2, 1]
    assert kv.nch[slots].tolist() == [3, 3, 3, 3, 2]  # columns: ceil((T + 17) / 32)
    assert kv.nshared[slots].tolist() == [2, 2, 2, 2, 0]
    # physical pages: entries 3 + 2 + 1, own 1 + 1 + 1 + 1 + 2 -- shared pages once; columns count them per holder
    assert kv.in_use == kv.peak == 12 and kv.pages_in_use() == 14
    assert kv.steps_reserved(slots) == 96 - 65
    # the tail copies: master tail -> the holder's first own page, for the contexts that end inside a page
    src, dst, rows = kv.tail_copies(slots)
    eA, eC = kv.entries[A], kv.entries[C]
    assert src.tolist() == [eA.pages[2], eA.pages[2], eC.pages[0]]
    assert dst.tolist() == [kv.host[4, 2], kv.host[0, 2], kv.host[1, 0]] and rows.tolist() == [1, 1, 31]
    every_entry_page = {int(p) for e in kv.entries.values() for p in e.pages}
    for s in slots:  # the page a slot appends into is never an entry's
        assert int(kv.host[s, kv.lens_host[s] // PAGE_ROWS]) not in every_entry_page
    assert len(set(dst.tolist())) == 3


@pytest.mark.parametrize("order", list(itertools.permutations(range(4))))
def test_release_in_every_order_returns_each_page_exactly_once(order):
    pool = _pool()
    kv = PagedKV(pool, 4, 0, 2)
    _admit(kv, [0, 1, 2, 3], [A, A, A, B_])  # B_ is held by one slot only: its entry leaves with it
    assert kv.in_use == 3 + 2 + 1 + 1 + 1 + 1
    for i, s in enumerate(order):
        kv.release([s])
        _check_books(kv, pool)
        left = [x for x in order[i + 1:] if x != 3]
        assert (A in kv.entries) == bool(left) and (B_ in kv.entries) == (3 in order[i + 1:])
    assert pool.free_pages == pool.total and kv.in_use == 0 and not kv.entries and kv.peak == 9


def test_a_released_holder_can_take_another_context_and_reuse_freed_pages():
    pool = _pool(seg_pages=1, budget_pages=10)
    kv = PagedKV(pool, 3, 0, 2)
    _admit(kv, [0, 1], [A, A])  # 3 + 1 + 1 pages
    _admit(kv, [2], [C])  # 1 + 2
    assert kv.in_use == 8
    kv.reset([0])  # A stays for slot 1
    _admit(kv, [0], [C])
    _check_books(kv, pool)
    assert kv.entries[C].holders == 2 and kv.entries[A].holders == 1 and kv.in_use == 9
    kv.reset([1])  # the last holder of A: its three pages are free again, and are what the next admission takes
    assert A not in kv.entries and kv.in_use == 5
    _admit(kv, [1], [B_])
    _check_books(kv, pool)
    assert pool.total <= 10
    kv.release([0, 1, 2])
    assert pool.free_pages == pool.total and not kv.entries


def test_hold_reports_a_full_pool_and_maps_nothing():
    pool = _pool(seg_pages=1, budget_pages=4)
    kv = PagedKV(pool, 3, 0, 2)
    kv.reset([0, 1, 2], lens=[65, 65, 64])
    failed = kv.hold([0, 1, 2], [A, A, B_], [65, 65, 64])  # A takes 3 of the 4 pages; B_ needs 2
    assert failed.tolist() == [2] and kv.nch.tolist() == [2, 2, 0] and kv.slot_entry[2] is None and B_ not in kv.entries
    _check_books(kv, pool)
    assert kv.ensure([0, 1], [66, 66]).tolist() == [1]  # one page left: slot 0's own tail page
    kv.release([1])
    _check_books(kv, pool)
    assert kv.entries[A].holders == 1
    kv.release([0])
    assert pool.free_pages == pool.total == 4
    assert kv.ensure([0], [10]).size == 0
    with pytest.raises(RuntimeError):
        kv.hold([0], [A], [65])  # a slot that still has pages cannot take a hold


def test_compact_keeps_shares():
    pool = _pool()
    kv = PagedKV(pool, 5, 0, 2)
    _admit(kv, [0, 1, 2, 3, 4], [A, C, A, B_, B_])
    rows = {s: kv.host[s].copy() for s in range(5)}
    kv.release([1, 3])
    kv.compact([4, 0, 2])
    assert kv.B == 3 and [e.key for e in kv.slot_entry] == [B_, A, A] and kv.nshared.tolist() == [2, 2, 2]
    assert (kv.host == np.stack([rows[4], rows[0], rows[2]])).all()
    _check_books(kv, pool)
    assert kv.entries[B_].holders == 1 and kv.entries[A].holders == 2 and C not in kv.entries
    assert kv.ensure([0, 1, 2], kv.lens_host + 40).size == 0  # own pages keep growing behind the shared ones
    _check_books(kv, pool)
    kv.release([1])
    kv.release([0, 2])
    assert pool.free_pages == pool.total and not kv.entries


def test_without_holds_nothing_changes_and_no_entry_exists():
    pool = _pool()
    kv = PagedKV(pool, 3, 0, 2)
    kv.reset([0, 1, 2], lens=[65, 33, 100])
    assert kv.ensure([0, 1, 2], np.array([65, 33, 100]) + 17).size == 0
    assert not kv.entries and kv.slot_entry == [None] * 3 and not kv.nshared.any()
    assert kv.in_use == kv.peak == kv.pages_in_use() == 3 + 2 + 4
    assert kv.tail_copies([0, 1, 2])[0].size == 0
    kv.release([0, 1, 2])
    assert pool.free_pages == pool.total and kv.in_use == 0


def test_multiplicity_is_counted_over_the_whole_call():
    ctxs = [list(A), list(C), list(A), list(B_)]
    keys, shares = _multiplicity(ctxs, True)
    assert keys == [A, None, A, None] and shares == [True, False, True, False]  # a singleton creates no entry
    assert _multiplicity(ctxs, False) == ([None] * 4, [False] * 4)


def test_sharing_keys_compare_whole_contexts_and_know_live_entries():
    near = list(A)
    near[7] += 1  # the length, first, middle and last id of A, another context
    assert sharing_keys([list(A), near, list(C)]) == [None, None, None]
    assert sharing_keys([list(A), near, list(A), list(C)]) == [A, None, A, None]
    assert sharing_keys([list(C), near], {C: None}) == [C, None]  # a live entry holds C
    assert sharing_keys([near], {A: None}) == [None]


def test_admission_estimate_counts_an_entry_once_per_batch_and_not_when_live():
    ctxs = [list(A), list(A), list(B_), list(A), list(C), list(B_)]
    keys, shares = _multiplicity(ctxs, True)
    assert shares == [True, True, True, True, False, True]
    ce = 16
    # own pages to T + 17: A 3 - 2 = 1, B_ 3 - 2 = 1, C (a singleton) 2; entries: A 3, B_ 2
    assert [own_pages(len(c), ce + 1, s) for c, s in zip(ctxs, shares)] == [1, 1, 1, 1, 2, 1]

    def admitted(room, live=(), nslots=6, sh=shares):
        return _admissible(deque(range(6)), ctxs, ce, nslots, room, keys, sh, live)

    # 3 + 1 | 1 | 2 + 1 | 1 | 2 | 1 = 12 pages for all six
    assert admitted(12) == [0, 1, 2, 3, 4, 5] and admitted(11) == [0, 1, 2, 3, 4]
    assert admitted(4) == [0] and admitted(3) == [] and admitted(5) == [0, 1] and admitted(7) == [0, 1]
    assert admitted(8) == [0, 1, 2]
    # a live entry costs nothing: 1 | 1 | 2 + 1 | 1 ...
    assert admitted(2, live={A: None}) == [0, 1] and admitted(5, live={A: None}) == [0, 1, 2]
    assert admitted(7, live={A: None, B_: None}) == [0, 1, 2, 3, 4, 5]
    assert admitted(12, nslots=2) == [0, 1]
    # sharing off: today's count, ceil((T + 17) / 32) each
    assert admitted(3 * 4 + 2 + 3, sh=None) == [0, 1, 2, 3, 4, 5] and admitted(16, sh=None) == [0, 1, 2, 3, 4]
    # the estimate is what the admission maps
    pool = _pool()
    kv = PagedKV(pool, 6, 0, 2)
    sl = np.arange(6)
    tl = np.asarray([len(c) for c in ctxs])
    kv.reset(sl, lens=tl)
    m = np.asarray(shares)
    assert kv.hold(sl[m], [k for k, s in zip(keys, shares) if s], tl[m]).size == 0
    assert kv.ensure(sl, tl + ce + 1).size == 0
    assert kv.in_use == 12
