"""CPU: the prefix planner and the chained page ownership of shared context prefixes (``lm/kvpages.py``) and the
admission estimate of the slot schedulers (``lm/slots.py``).  Different contexts of a call that begin with the same 64-token blocks hold one PREFIX entry per maximal run of blocks; a holder's table row is the chain's
pages, then its context's entry's full pages if it has one, then its own.  Every page goes back to the pool exactly
once, whatever the order of releases; the device side is covered by ``tests/test_gpu_prefix_prefill.py`` and
``tests/test_gpu_prefix_share.py``."""

import itertools
from collections import deque

import numpy as np
import pytest
import torch

from neuralsteganography_amd.lm.kvpages import (KVPagePool, PagedKV, chain_past, own_pages, plan_prefixes,
                                                   shared_pages, sharing_keys)
from neuralsteganography_amd.lm.slots import _admissible, _map_contexts


def context_set(seed=5):
    """The A..G set: ``base`` is 130 random ids; A and B carry its first 128, C its first 64, D none, E equals A and
    G is the first 128 exactly."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 511, size=130).tolist()
    ctx = {"A": base[:128] + rng.integers(0, 511, size=5).tolist(),
           "B": base[:128] + rng.integers(0, 511, size=40).tolist(),
           "C": base[:64] + rng.integers(0, 511, size=30).tolist(),
           "D": rng.integers(0, 511, size=70).tolist()}
    ctx["E"] = list(ctx["A"])
    ctx["G"] = base[:128]
    return base, ctx


NAMES = "ABCDEG"
BASE, CTX = context_set()
RUN1, RUN2 = tuple(BASE[:64]), tuple(BASE[:128])


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


def test_planner_finds_the_two_runs_and_each_contexts_past():
    chains = dict(zip(NAMES, plan_prefixes([CTX[k] for k in NAMES])))
    one, two = (RUN1, 0, 64), (RUN2, 64, 128)
    assert chains["A"] == chains["B"] == chains["E"] == (one, two)
    assert chains["C"] == (one,) and chains["D"] == ()
    assert chains["G"] == (one,)  # 64, not 128: a new row must remain
    assert {k: chain_past(c) for k, c in chains.items()} == {"A": 128, "B": 128, "C": 64, "D": 0, "E": 128, "G": 64}
    # the runs' holders: the first by A, B, C, E and G, the second by A, B and E
    assert sorted(k for k, c in chains.items() if one in c) == list("ABCEG")
    assert sorted(k for k, c in chains.items() if two in c) == list("ABE")
    # A and E are the same context: an equal-context entry, as in 0.30, now beneath the second run
    keys = sharing_keys([CTX[k] for k in NAMES])
    assert [k is not None for k in keys] == [True, False, False, False, True, False] and keys[0] == tuple(CTX["A"])


def test_planner_leaves_short_equal_and_unrelated_contexts_alone():
    rng = np.random.default_rng(9)
    b = rng.integers(0, 511, size=64).tolist()
    # 64 tokens or fewer: past 0, whatever else begins with them
    assert plan_prefixes([b, b + [1, 2], b[:40]]) == [(), (), ()]
    # two copies of ONE context are no two distinct contexts: that is the equal-context entry's business
    assert plan_prefixes([b + [1], b + [1]]) == [(), ()]
    assert plan_prefixes([b + [1], b + [2]]) == [((tuple(b), 0, 64),)] * 2
    # a difference inside the first block: nothing to share
    assert plan_prefixes([b + [1], b[:63] + [b[63] ^ 1, 1]]) == [(), ()]
    many = [rng.integers(0, 50257, size=int(n)).tolist() for n in rng.integers(65, 1023, size=256)]
    assert plan_prefixes(many) == [()] * 256


def test_planner_bounds_a_chain_at_two_runs():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 511, size=256).tolist()
    ctxs = [b[:64 * k] + [600 + k] for k in (1, 2, 3, 4)] + [b[:256] + [700]]
    chains = plan_prefixes(ctxs)
    assert [chain_past(c) for c in chains] == [64, 128, 128, 128, 128]
    assert all(len(c) <= 2 for c in chains)


def _admit(kv, names, slots, ahead=17):
    """What a scheduler's admission does: plan over the whole set, hold chains and entries, map own pages."""
    ctxs = [CTX[k] for k in NAMES]
    chains = dict(zip(NAMES, plan_prefixes(ctxs)))
    keys = dict(zip(NAMES, sharing_keys(ctxs)))
    slots = np.asarray(slots)
    tl = np.asarray([len(CTX[k]) for k in names])
    ok = _map_contexts(kv, slots, [keys[k] for k in names], [keys[k] is not None for k in names], tl, tl + ahead,
                       [chains[k] for k in names])
    assert ok.all()


def _check_books(kv, pool):
    """Every page of the pool is free, an entry's, or in exactly one slot's own columns; holders add up."""
    tab = kv.host
    assert (kv.table.numpy() == tab).all()
    own = [int(p) for s in range(kv.B) for p in tab[s, kv.nshared[s]: kv.nch[s]]]
    everyone = list(kv.entries.values()) + list(kv.prefixes.values())
    ent = [int(p) for e in everyone for p in e.pages]
    free = pool._free[: pool.free_pages].tolist()
    everything = own + ent + free
    assert len(everything) == pool.total and len(set(everything)) == pool.total and 0 not in everything
    assert kv.in_use == len(own) + len(ent)
    for e in everyone:
        slots = sum(1 for x in list(kv.slot_entry) + list(kv.slot_prefix) if x is e)
        assert e.holders == slots + sum(1 for x in everyone if x.parent is e) and e.holders > 0
        assert e.past == (e.parent.T if e.parent is not None else 0)
    for s in range(kv.B):
        e = kv.slot_entry[s] or kv.slot_prefix[s]
        want = e.table_pages().tolist() if e is not None else []
        assert kv.nshared[s] == len(want) and tab[s, : len(want)].tolist() == want
        assert not tab[s, kv.nch[s]:].any()


def test_table_rows_are_the_chain_then_the_entry_then_own_pages():
    pool = _pool()
    kv = PagedKV(pool, 6, 0, 2)
    slots = [4, 0, 2, 5, 1, 3]
    _admit(kv, NAMES, slots)
    _check_books(kv, pool)
    p1, p2, eA = kv.prefixes[RUN1], kv.prefixes[RUN2], kv.entries[tuple(CTX["A"])]
    assert set(kv.prefixes) == {RUN1, RUN2} and set(kv.entries) == {tuple(CTX["A"])}
    assert (p1.past, p1.T, p1.pages.size, p1.parent) == (0, 64, 2, None)
    assert (p2.past, p2.T, p2.pages.size, p2.parent) == (64, 128, 2, p1)
    assert (eA.past, eA.T, eA.parent, eA.full, eA.tail_rows, eA.pages.size) == (128, 133, p2, 0, 5, 1)
    # holders: p1 by p2 and the slots of C and G; p2 by A's entry and the slot of B; the entry by A and E
    assert (p1.holders, p2.holders, eA.holders) == (3, 2, 2)
    row = dict(zip(NAMES, slots))
    chain2 = p1.pages.tolist() + p2.pages.tolist()
    for k in "ABE":
        assert kv.host[row[k], :4].tolist() == chain2 and kv.nshared[row[k]] == 4
    for k in "CG":
        assert kv.host[row[k], :2].tolist() == p1.pages.tolist() and kv.nshared[row[k]] == 2
    assert kv.nshared[row["D"]] == 0 and kv.slot_entry[row["D"]] is None and kv.slot_prefix[row["D"]] is None
    # columns: ceil((T + 17) / 32)
    assert kv.nch[slots].tolist() == [-(-(len(CTX[k]) + 17) // 32) for k in NAMES]
    # physical pages: 2 + 2 (runs) + 1 (A's master tail), own A 1, B 2, C 2, D 3, E 1, G 3 -- a shared page once
    assert kv.in_use == kv.peak == 5 + 12 and kv.pages_in_use() == int(kv.nch.sum())
    # private, the same six contexts map sum(ceil((T + 17) / 32)) pages
    assert kv.in_use < sum(-(-(len(CTX[k]) + 17) // 32) for k in NAMES)
    # the master tail of the equal-context entry goes to column base + full of each holder
    src, dst, rows = kv.tail_copies(slots)
    assert src.tolist() == [eA.pages[0]] * 2 and rows.tolist() == [5, 5]
    assert dst.tolist() == [kv.host[row["A"], 4], kv.host[row["E"], 4]]


@pytest.mark.parametrize("order", list(itertools.permutations(range(6)))[::37])
def test_releases_in_any_order_return_every_page(order):
    pool = _pool()
    kv = PagedKV(pool, 6, 0, 2)
    _admit(kv, NAMES, np.arange(6))
    total = pool.total
    for s in order:
        kv.release([s])
        _check_books(kv, pool)
    assert kv.in_use == 0 and not kv.entries and not kv.prefixes and pool.free_pages == pool.total == total
    assert not kv.host.any() and not kv.table.any()


def test_a_prefix_is_opened_again_after_its_last_holder_left():
    pool = _pool()
    kv = PagedKV(pool, 3, 0, 2)
    _admit(kv, "BC", [0, 1])
    assert kv.prefixes[RUN1].holders == 2 and kv.prefixes[RUN2].holders == 1
    kv.release([0])  # B leaves: the second run goes with it, the first stays for C
    assert set(kv.prefixes) == {RUN1} and kv.prefixes[RUN1].holders == 1
    _check_books(kv, pool)
    kv.prefixes[RUN1].ready = True
    _admit(kv, "A", [2])  # A arrives: the live first run is held, the second and A's entry are new
    assert kv.prefixes[RUN1].ready and not kv.prefixes[RUN2].ready and kv.prefixes[RUN1].holders == 2
    _check_books(kv, pool)
    kv.release([1, 2])
    assert kv.in_use == 0 and not kv.prefixes and not kv.entries and pool.free_pages == pool.total


def test_a_short_pool_maps_nothing_for_the_slot_it_cannot_serve():
    pool = _pool(seg_pages=4, budget_pages=4)
    kv = PagedKV(pool, 2, 0, 2)
    ctxs = [CTX[k] for k in NAMES]
    chains = dict(zip(NAMES, plan_prefixes(ctxs)))
    tl = np.asarray([len(CTX["B"]), len(CTX["C"])])
    # B needs 2 + 2 chain pages and 2 own: the 4-page pool serves the chain and then has no page for B's own, nor
    # for C's (which holds the live first run): both are left released, and the runs leave with them
    ok = _map_contexts(kv, np.arange(2), [None, None], [False, False], tl, tl + 17, [chains["B"], chains["C"]])
    assert ok.tolist() == [False, False]
    assert not kv.nch.any() and kv.slot_prefix == [None, None] and not kv.prefixes and kv.in_use == 0
    _check_books(kv, pool)
    kv.release([0, 1])
    assert kv.in_use == 0 and not kv.prefixes and pool.free_pages == pool.total


def test_admission_counts_a_prefix_once_with_its_opener():
    ctxs = [CTX[k] for k in NAMES]
    chains, keys = plan_prefixes(ctxs), sharing_keys(ctxs)
    shares = [k is not None for k in keys]
    ahead = 16
    own = {k: own_pages(len(CTX[k]), ahead + 1, s, chain_past(c)) for k, s, c in zip(NAMES, shares, chains)}
    assert own == {"A": 1, "B": 2, "C": 2, "D": 3, "E": 1, "G": 3}
    assert shared_pages(64, 0) == shared_pages(128, 64) == 2 and shared_pages(133, 128) == 1
    # A opens both runs and its entry: 1 + 2 + 2 + 1; B then needs its own 2 only; C 2; D 3; E 1; G 3
    need = [6, 2, 2, 3, 1, 3]
    for n in range(1, 7):
        room = sum(need[:n])
        q = deque(range(6))
        assert _admissible(q, ctxs, ahead, 6, room, keys, shares, (), chains, ()) == list(range(n))
        q = deque(range(6))
        assert _admissible(q, ctxs, ahead, 6, room - 1, keys, shares, (), chains, ()) == list(range(n - 1))
    # live runs are not counted again; a live entry's chain is live with it
    q = deque([1, 2])
    assert _admissible(q, ctxs, ahead, 6, 4, keys, shares, (), chains, (RUN1, RUN2)) == [1, 2]
    q = deque([4])
    assert _admissible(q, ctxs, ahead, 6, 1, keys, shares, (keys[0],), chains, (RUN1, RUN2)) == [4]
    # the estimate is what the admission maps
    pool = _pool()
    kv = PagedKV(pool, 6, 0, 2)
    _admit(kv, NAMES, np.arange(6), ahead=ahead + 1)
    assert kv.in_use == sum(need)
    # without chains the arithmetic is 0.30's
    q = deque(range(6))
    old = [own_pages(len(c), ahead + 1, s) + (shared_pages(len(c)) if i == 0 else 0)
           for i, (c, s) in enumerate(zip(ctxs, shares))]
    assert _admissible(q, ctxs, ahead, 6, sum(old), keys, shares, ()) == list(range(6)) and sum(old) > sum(need)
