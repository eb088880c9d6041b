"""Paged KV cache of the native decode step (round 6): 32-position pages owned per stream.

The reference keeps one unbounded KV cache per message and runs every message in its own loop
(``code_base/arithmetic.py:96-122``; ``limit_past`` is a no-op, ``code_base/utils.py:19-30``).  Batched, that is B
caches of different, unknown lengths.  A dense ``[B, longest]`` allocation wastes the memory of every short
stream and must be copied to grow; here a stream's rows live in pages it owns:

* a PAGE holds 32 positions of one stream for every layer, ``[K|V][H][32][D]`` per layer in the cache's element
  type (1.18 MB for GPT-2-small fp16 over its 12 layers), so the attention of one (stream, head) reads 4 KiB
  contiguous per page and layer; pages live in SEGMENTS of ``seg_pages`` pages stored layer-major,
  ``[layer][page][K|V][H][32][D]``, so one layer's pages are contiguous (a decode step's attention walks one layer
  at a time: as few address-translation regions per launch as the dense cache had -- pages that interleave the
  layers measured 3-22 % slower, ``tools/paged_attn_probe.py``); a page's table entry is its layer-0 block's
  address and layer ``i`` is ``i * seg_pages * block`` elements further;
* the page TABLE ``[B, width]`` (uint64 device addresses, 0 = none) maps a stream's row ``r`` (position ``T0 + r``)
  to page ``table[b, r // 32]`` -- ``ns_decode_attention_paged`` reads it; per-stream cache lengths ``lens[B]``
  (int32, device) feed the position embedding and the attention and are advanced by the step's final layer norm;
* the POOL hands out pages from segments allocated on demand and kept across calls (warm pages); growth maps new
  segments and never copies a filled page, and a stream's pages return to the pool when it ends, so the memory in
  use follows the live tokens, not B x the longest stream.  When the device has no room for another segment the
  pool reports it (:class:`KVCapacityError` upstream), never PyTorch's out-of-memory.

SHARED CONTEXTS (library 0.30).  With one context per message, the messages of a call that carry the same context
share its full pages read-only: a :class:`SharedContext` entry of the call's registry (``PagedKV.entries``, keyed by
the trimmed context as a tuple) owns ``ceil(T / 32)`` pages -- the ``T // 32`` full ones and, when ``r = T % 32 > 0``,
a MASTER TAIL page that no slot ever appends into.  A holder's table row has the entry's full pages in its first
``T // 32`` columns and its own pages after them; the first own page receives the master tail's ``r`` rows as a copy
(``ns_kv_copy_rows``), because the slot appends into that page from row ``r`` on.  :meth:`PagedKV.release` returns a
slot's own pages only and drops its hold; the entry's pages go back to the pool with its last holder, and nothing is
kept for later.  ``in_use`` / ``peak`` count physical pages (a shared page once); ``nch`` counts table columns.

SHARED PREFIXES.  Different contexts of a call that begin with the same tokens share the pages of
that beginning, in units of 64 rows (two pages: the key block of the prefill's attention, which is what keeps the bits
equal -- ``ns_seq_attention_ragged_past``).  :func:`plan_prefixes` builds a trie over the 64-token blocks of the
call's distinct contexts; a PREFIX ENTRY (``PagedKV.prefixes``, keyed by the tokens up to its end) is a maximal run of
blocks that one set of at least two distinct contexts passes through, its ``parent`` the run before it, and a
context's ``past`` -- the rows it does not prefill -- is the end of its deepest run, always below its length.  A
prefix entry owns its own run's pages only (all full: no master tail, no copy); an equal-context entry may have a
prefix parent and then owns the pages after it.  A holder's table row is the chain's pages in order, then the
equal-context entry's full pages if there is one, then its own.  Entries count their holders -- slots, and the
entries opened beneath them -- so holds and releases walk the chain and an entry's pages return to the pool with its
last holder.  A chain is at most ``MAX_PREFIX_DEPTH`` = 2 runs deep; what a context shares beyond them stays private.
fp8 pages hold converted values, not the bits a whole prefill attends over, so prefixes are shared with fp16 pages only.

The host keeps a mirror of the table and of the lengths (every slot advances one position per step), so page
bookkeeping needs no device read.  Pure host logic over torch tensors: the CPU tests drive it with CPU tensors.
"""

from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

PAGE_ROWS = 32
PREFIX_ROWS = 64  # a shared prefix ends on a key block of the prefill's attention (two pages)
MAX_PREFIX_DEPTH = 2  # prefix entries on one context's chain


class KVPagePool:
    """Pages in layer-major segments of ``seg_pages`` pages each; a free list of page (layer-0 block) addresses.

    ``budget_bytes()`` says how much more device memory the pool may take (free memory minus what the caller must
    keep free); growth asks for ``max(needed, total / 4)`` pages, in whole segments, within that budget."""

    def __init__(self, n_layer: int, n_head: int, head_dim: int, dtype: torch.dtype, device,
                 budget_bytes: Optional[Callable[[], int]] = None, seg_pages: int = 1024):
        self.n_layer = int(n_layer)
        self.block_elems = 2 * n_head * PAGE_ROWS * head_dim  # one layer's [K|V][H][32][D]
        self.page_elems = self.n_layer * self.block_elems
        self.esize = torch.tensor([], dtype=dtype).element_size()
        self.block_bytes = self.block_elems * self.esize
        self.page_bytes = self.page_elems * self.esize
        self.dtype, self.device = dtype, torch.device(device)
        self.budget_bytes = budget_bytes
        self.seg_pages = max(1, int(seg_pages))
        self.segments: List[torch.Tensor] = []
        self._free = np.empty(0, dtype=np.int64)
        self._nfree = 0
        self.total = 0

    # ------------------------------------------------------------------
    def layer_offset(self, layer: int) -> int:
        """Elements from a page's address to its block of ``layer`` (``ns_decode_attention_paged``)."""
        return int(layer) * self.seg_pages * self.block_elems

    @property
    def free_pages(self) -> int:
        return self._nfree

    def growable_pages(self) -> int:
        if self.budget_bytes is None:
            return 1 << 40
        return max(0, int(self.budget_bytes()) // self.page_bytes)

    def _addresses(self, seg: torch.Tensor) -> np.ndarray:
        return seg.data_ptr() + self.block_bytes * np.arange(self.seg_pages, dtype=np.int64)

    def add_segment(self, npages: int) -> bool:
        """Map at least ``npages`` more pages (whole segments, one allocation each); False (nothing mapped) if the
        device cannot hold them."""
        nseg = -(-int(npages) // self.seg_pages)
        if nseg <= 0:
            return False
        new = []
        for _ in range(nseg):
            try:
                new.append(torch.empty((self.n_layer, self.seg_pages, self.block_elems), dtype=self.dtype,
                                       device=self.device))
            except torch.OutOfMemoryError:
                return False
        for seg in new:
            self.segments.append(seg)
            self._push(self._addresses(seg)[::-1])  # pages are taken from the top: lowest addresses first
            self.total += self.seg_pages
        return True

    def _push(self, addrs: np.ndarray) -> None:
        n = addrs.size
        if self._nfree + n > self._free.size:
            grown = np.empty(max(self._nfree + n, 2 * self._free.size), dtype=np.int64)
            grown[: self._nfree] = self._free[: self._nfree]
            self._free = grown
        self._free[self._nfree: self._nfree + n] = addrs
        self._nfree += n

    def take(self, n: int) -> Optional[np.ndarray]:
        """``n`` page addresses, growing the pool within its budget; None (nothing taken) if it cannot."""
        n = int(n)
        if n <= 0:
            return np.empty(0, dtype=np.int64)
        if self._nfree < n:
            short = n - self._nfree
            room = self.growable_pages() // self.seg_pages * self.seg_pages
            if room < short:
                return None
            want = min(room, max(short, self.total // 4))
            if not self.add_segment(want) and not (want > short and self.add_segment(short)):
                return None
        out = self._free[self._nfree - n: self._nfree][::-1].copy()
        self._nfree -= n
        return out

    def give(self, addrs: np.ndarray) -> None:
        addrs = np.asarray(addrs, dtype=np.int64)
        if addrs.size:
            self._push(addrs[::-1])

    def reset(self) -> None:
        """Every page free again (a new call: the previous call's tables are dropped)."""
        self._free = np.empty(0, dtype=np.int64)
        self._nfree = 0
        for seg in self.segments:
            self._push(self._addresses(seg)[::-1])

    def release_memory(self) -> None:
        self.segments = []
        self._free = np.empty(0, dtype=np.int64)
        self._nfree = 0
        self.total = 0


class SharedContext:
    """One context's KV pages held by several slots of a call (see the module docstring): ``pages`` are its
    ``ceil(T / 32)`` page addresses (the last one the master tail when ``tail_rows > 0``), ``logits`` the ``[1, ld]``
    row after the context's last token (None until the entry has been prefilled), ``holders`` the slots holding it.

    With a ``parent`` (a prefix entry) the entry owns rows ``past .. T-1`` only, ``past`` = the parent's
    ``T``: ``pages`` are the ``ceil(T / 32) - past / 32`` pages after the parent's, ``full`` counts the full ones among
    them and ``base`` the table columns before them.  A PREFIX entry (``is_prefix``: rows ``past .. T-1`` of every
    context that begins with ``key``, both multiples of 64) has full pages only and no logits; ``ready`` says its rows
    have been prefilled.  ``holders`` counts slots and the entries opened beneath this one."""

    __slots__ = ("key", "T", "pages", "full", "tail_rows", "logits", "holders", "parent", "past", "is_prefix", "ready")

    def __init__(self, key, T: int, pages: np.ndarray, parent: "SharedContext" = None, is_prefix: bool = False):
        self.key, self.T, self.pages = key, int(T), pages
        self.parent, self.past = parent, (parent.T if parent is not None else 0)
        self.full, self.tail_rows = (self.T - self.past) // PAGE_ROWS, self.T % PAGE_ROWS
        self.is_prefix, self.ready = bool(is_prefix), False
        self.logits = None
        self.holders = 0

    @property
    def base(self) -> int:
        """Table columns before this entry's pages (its chain's)."""
        return self.past // PAGE_ROWS

    def table_pages(self, tail: bool = False) -> np.ndarray:
        """The chain's pages in order, then this entry's full pages (``tail``: its master tail too)."""
        own = self.pages if tail else self.pages[: self.full]
        return own if self.parent is None else np.concatenate([self.parent.table_pages(), own])


def sharing_keys(contexts, entries=()):
    """For every context of a call its registry key (the context as a tuple) if it shares -- another context of the
    list equals it, or a live entry of ``entries`` holds it -- else None.  Only candidates (equal length, first, middle
    and last id) are turned into tuples and hashed: a call of distinct contexts pays a few operations per context."""
    def sig(c):
        return (len(c), c[0], c[len(c) // 2], c[-1])

    sigs = [sig(c) for c in contexts]
    seen = {}
    for g in sigs:
        seen[g] = seen.get(g, 0) + 1
    live = {sig(k) for k in entries}
    keys = [tuple(c) if seen[g] > 1 or g in live else None for c, g in zip(contexts, sigs)]
    count = {}
    for k in keys:
        if k is not None:
            count[k] = count.get(k, 0) + 1
    return [k if k is not None and (count[k] > 1 or k in entries) else None for k in keys]


def plan_prefixes(contexts):
    """For every (trimmed) context of a call its CHAIN of shared prefix runs, outermost first: a tuple of
    ``(key, start, end)`` -- rows ``start .. end-1`` (multiples of 64) of every context that begins with ``key``, the
    context's first ``end`` ids -- or ``()`` when it shares no prefix.  A run is a maximal stretch of 64-token blocks
    that one set of at least 2 DISTINCT contexts passes through (a context passes through the blocks that end below
    its length: one new row always remains); at most ``MAX_PREFIX_DEPTH`` runs per chain, the rest stays private.  A
    context of 64 tokens or fewer has none.  Only contexts whose first block looks like another's (ids 0, 31 and 63)
    enter the trie: a call of unrelated contexts pays a few operations per context."""
    chains = [()] * len(contexts)

    def sig(c):
        return (c[0], c[31], c[63])

    seen = {}
    for c in contexts:
        if len(c) > PREFIX_ROWS:
            g = sig(c)
            seen[g] = seen.get(g, 0) + 1
    distinct = {}
    for i, c in enumerate(contexts):
        if len(c) > PREFIX_ROWS and seen[sig(c)] > 1:
            distinct.setdefault(tuple(c), []).append(i)
    if len(distinct) < 2:
        return chains
    nodes, paths = {}, []  # (parent node, block) -> [node id, distinct contexts through it]
    for c in distinct:
        pid, path = 0, []
        for k in range((len(c) - 1) // PREFIX_ROWS):
            node = nodes.setdefault((pid, c[PREFIX_ROWS * k: PREFIX_ROWS * (k + 1)]), [len(nodes) + 1, 0])
            node[1] += 1
            pid = node[0]
            path.append(node)
        paths.append(path)
    for (c, who), path in zip(distinct.items(), paths):
        chain, k = [], 0
        while k < len(path) and path[k][1] >= 2 and len(chain) < MAX_PREFIX_DEPTH:
            j = k
            while j < len(path) and path[j][1] == path[k][1]:  # the same set: sets only shrink along a path
                j += 1
            chain.append((c[: PREFIX_ROWS * j], PREFIX_ROWS * k, PREFIX_ROWS * j))
            k = j
        for i in who:
            chains[i] = tuple(chain)
    return chains


def chain_past(chain) -> int:
    """Rows a context with this chain does not prefill: the end of its deepest shared run."""
    return int(chain[-1][2]) if chain else 0


def shared_pages(T: int, past: int = 0) -> int:
    """Pages a shared context of ``T`` rows owns: its full pages and the master tail (after its prefix parent's
    ``past`` rows, if it has one); a prefix run of rows ``past .. T-1`` owns ``(T - past) / 32``."""
    return (int(T) + PAGE_ROWS - 1) // PAGE_ROWS - int(past) // PAGE_ROWS


def own_pages(T: int, ahead: int, shares: bool, past: int = 0) -> int:
    """Pages a message with a ``T``-row context maps for itself up to position ``T + ahead``: all of them, or, when it
    shares the context, those after the context's full pages, or, when it shares a prefix of ``past`` rows only,
    those after the prefix."""
    need = (int(T) + int(ahead) + PAGE_ROWS - 1) // PAGE_ROWS
    return need - int(T) // PAGE_ROWS if shares else need - int(past) // PAGE_ROWS


class PagedKV:
    """One call's page table, per-stream lengths and their host mirrors over a :class:`KVPagePool`.

    Slots are rows ``0..B-1``.  ``lens`` (device int32) is advanced by the decode step itself; the host mirror
    ``lens_host`` is advanced by :meth:`advance` (every slot moves one position per step, finished ones too: their
    attention is skipped, their length only feeds the position embedding of rows nobody reads).  ``version`` changes
    whenever a device tensor is replaced (a wider table, a compaction): a captured graph must then be re-captured."""

    def __init__(self, pool: KVPagePool, B: int, T0: int, width: int):
        self.pool, self.B, self.T0 = pool, int(B), int(T0)
        dev = pool.device
        self.width = max(1, int(width))
        self.table = torch.zeros((self.B, self.width), dtype=torch.int64, device=dev)
        self.host = np.zeros((self.B, self.width), dtype=np.int64)
        self.nch = np.zeros(self.B, dtype=np.int64)
        self.lens = torch.full((self.B,), self.T0, dtype=torch.int32, device=dev)
        self.lens_host = np.full(self.B, self.T0, dtype=np.int64)
        self.version = 0
        self.in_use = 0  # physical pages mapped now (a shared page once), and the most at once in this call
        self.peak = 0
        self.entries = {}  # trimmed context (tuple) -> SharedContext, while at least one slot holds it
        self.prefixes = {}  # a shared prefix's tokens (tuple) -> its SharedContext, while anything holds it
        self.slot_entry: List[Optional[SharedContext]] = [None] * self.B
        self.slot_prefix: List[Optional[SharedContext]] = [None] * self.B  # a private suffix's deepest prefix entry
        self.nshared = np.zeros(self.B, dtype=np.int64)  # leading table columns that are an entry's pages

    # ------------------------------------------------------------------
    def pages_in_use(self) -> int:
        return int(self.nch.sum())

    def _grow_width(self, need: int) -> None:
        w = max(int(need), 2 * self.width)
        t = torch.zeros((self.B, w), dtype=torch.int64, device=self.table.device)
        t[:, : self.width] = self.table
        h = np.zeros((self.B, w), dtype=np.int64)
        h[:, : self.width] = self.host
        self.table, self.host, self.width = t, h, w
        self.version += 1

    def ensure(self, slots, upto) -> np.ndarray:
        """Give every slot in ``slots`` the pages for positions below ``upto`` (scalar or per slot).  All or nothing
        per slot; returns the slots that could not be served (the pool is out of memory)."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if slots.size == 0:
            return slots
        upto = np.broadcast_to(np.asarray(upto, dtype=np.int64), slots.shape)
        need = np.maximum(0, (upto - self.T0 + PAGE_ROWS - 1) // PAGE_ROWS)
        deficit = np.maximum(0, need - self.nch[slots])
        if not deficit.any():
            return np.empty(0, dtype=np.int64)
        if int(need.max()) > self.width:
            self._grow_width(int(need.max()))
        pages = self.pool.take(int(deficit.sum()))
        if pages is not None:
            self._assign(slots, deficit, pages)
            return np.empty(0, dtype=np.int64)
        failed = []
        for s, d in zip(slots.tolist(), deficit.tolist()):  # the pool is short: serve slots in order while it lasts
            if d == 0:
                continue
            p = self.pool.take(d)
            if p is None:
                failed.append(s)
            else:
                self._assign(np.array([s]), np.array([d]), p)
        return np.asarray(failed, dtype=np.int64)

    def _assign(self, slots: np.ndarray, deficit: np.ndarray, pages: np.ndarray) -> None:
        keep = deficit > 0
        slots, deficit = slots[keep], deficit[keep]
        rows = np.repeat(slots, deficit)
        starts = np.repeat(np.cumsum(deficit) - deficit, deficit)
        cols = self.nch[rows] + (np.arange(rows.size) - starts)
        self.host[rows, cols] = pages
        self.nch[slots] += deficit
        self.in_use += int(pages.size)
        self.peak = max(self.peak, self.in_use)
        dev = self.table.device
        self.table[torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)] = torch.from_numpy(pages).to(dev)

    def hold(self, slots, keys, lens, chains=None) -> np.ndarray:
        """Let every slot in ``slots`` (released, no page mapped) hold the shared context ``keys[i]`` of ``lens[i]``
        rows: the entry is opened if no slot holds it yet (its pages taken from the pool; its ``logits`` stay None
        until the caller has prefilled it), and its full pages become the slot's first table columns.  The slot's own
        pages follow through :meth:`ensure`.  ``chains[i]`` (:func:`plan_prefixes`) names the context's shared prefix
        runs: those not live are opened with the entry (``ready`` False until prefilled), each the parent of the
        next and the last the parent of the context's entry; with ``keys[i]`` None the slot holds the deepest run
        itself and its private suffix follows in its own pages.  The table row is the chain's pages, then the entry's.
        Returns the slots for which something could not be opened (the pool is out of memory); nothing is mapped for
        them."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        failed, rows, cols, pages = [], [], [], []
        lens = np.asarray(lens, dtype=np.int64).reshape(-1).tolist()
        for i, (s, key, T) in enumerate(zip(slots.tolist(), keys, lens)):
            if self.nch[s] or self.slot_entry[s] is not None or self.slot_prefix[s] is not None:
                raise RuntimeError("hold: the slot still has pages")
            e = self.entries.get(key) if key is not None else None
            if e is None:
                chain = chains[i] if chains is not None else ()
                if key is None and not chain:
                    raise ValueError("hold: neither a shared context nor a shared prefix")
                if chain and chain[-1][2] >= T:
                    raise ValueError("hold: a shared prefix must end below the context's length")
                e = self._open(key, T, chain)
                if e is None:
                    failed.append(s)
                    continue
            elif e.T != T:
                raise ValueError("hold: the context's length differs from its entry's")
            e.holders += 1
            if e.is_prefix:
                self.slot_prefix[s] = e
            else:
                self.slot_entry[s] = e
            tp = e.table_pages()
            self.nshared[s] = self.nch[s] = tp.size
            rows.append(np.full(tp.size, s, dtype=np.int64))
            cols.append(np.arange(tp.size, dtype=np.int64))
            pages.append(tp)
        if rows:
            rows, cols, pages = np.concatenate(rows), np.concatenate(cols), np.concatenate(pages)
            if rows.size:
                if int(cols.max()) + 1 > self.width:
                    self._grow_width(int(cols.max()) + 1)
                self.host[rows, cols] = pages
                dev = self.table.device
                self.table[torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)] = \
                    torch.from_numpy(pages).to(dev)
        return np.asarray(failed, dtype=np.int64)

    def _open(self, key, T: int, chain) -> Optional[SharedContext]:
        """Open what a holder of context ``key`` (None: a private suffix) with ``chain`` needs and nothing holds yet
        -- the chain's runs that are not live, then the context's entry -- with ONE take from the pool (all or
        nothing).  Returns the entry the holder holds (no hold counted yet), or None if the pool is short."""
        todo, past = [], 0
        for k, a, b in chain:
            p = self.prefixes.get(k)
            if a != past or b <= a or b % PREFIX_ROWS or (p is not None and (p.past, p.T) != (a, b)):
                raise ValueError("hold: the shared prefix chain does not fit its live entries")
            if p is None:
                todo.append((k, b, a, True))
            past = b
        if key is not None:
            todo.append((key, T, past, False))
        taken = self.pool.take(sum(shared_pages(t, a) for _, t, a, _ in todo))
        if taken is None:
            return None
        self.in_use += int(taken.size)
        self.peak = max(self.peak, self.in_use)
        live = len(chain) - sum(1 for t in todo if t[3])  # live runs are the chain's head: a run holds its parent
        e = self.prefixes[chain[live - 1][0]] if live else None
        for k, t, a, is_prefix in todo:
            n = shared_pages(t, a)
            child = SharedContext(k, t, taken[:n], parent=e, is_prefix=is_prefix)
            taken = taken[n:]
            if e is not None:
                e.holders += 1
            (self.prefixes if is_prefix else self.entries)[k] = child
            e = child
        return e

    def tail_copies(self, slots):
        """``(src, dst, rows)`` for ``ns_kv_copy_rows``: for every holder in ``slots`` whose context ends inside a
        page, the entry's master tail page, the slot's first own page (mapped) and the rows to copy."""
        src, dst, rows = [], [], []
        for s in np.asarray(slots, dtype=np.int64).reshape(-1).tolist():
            e = self.slot_entry[s]
            if e is None or e.tail_rows == 0:
                continue
            if self.nch[s] <= e.base + e.full:
                raise RuntimeError("tail_copies: the holder's first own page is not mapped")
            src.append(int(e.pages[e.full]))
            dst.append(int(self.host[s, e.base + e.full]))
            rows.append(e.tail_rows)
        return (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(rows, dtype=np.int32))

    def release(self, slots) -> None:
        """Return the own pages of ``slots`` to the pool and clear their table rows (the streams have ended); a slot
        that held a shared context drops its hold, and the entry's pages follow its last holder."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if slots.size == 0:
            return
        n = int(self.nch[slots].max(initial=0))
        if n:
            pages = self.host[slots, :n]
            pages = pages[(pages != 0) & (np.arange(n)[None, :] >= self.nshared[slots][:, None])]
            self.pool.give(pages)
            self.in_use -= int(pages.size)
            self.host[slots, :n] = 0
            self.table[torch.from_numpy(slots).to(self.table.device), :n] = 0
        self.nch[slots] = 0
        self.nshared[slots] = 0
        for s in slots.tolist():
            e = self.slot_entry[s] or self.slot_prefix[s]
            self.slot_entry[s] = self.slot_prefix[s] = None
            while e is not None:  # up the chain while an entry loses its last holder
                e.holders -= 1
                if e.holders:
                    break
                self.pool.give(e.pages)  # nothing is kept for later: the page budget stays exact
                self.in_use -= int(e.pages.size)
                del (self.prefixes if e.is_prefix else self.entries)[e.key]
                e = e.parent

    def reset(self, slots, lens=None) -> None:
        """``release`` + the slots' cache lengths back to the shared context (a new message starts there), or to
        ``lens`` (one length per slot, >= ``T0``: a message whose own context of ``lens - T0`` rows is about to be
        prefilled into its pages; the caller maps them with :meth:`ensure`)."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        self.release(slots)
        self.set_lens(slots, self.T0 if lens is None else lens)

    def set_lens(self, slots, lens) -> None:
        """Cache lengths of ``slots`` (scalar or one per slot, >= ``T0``), on the device and in the host mirror."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if slots.size == 0:
            return
        lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), slots.shape)
        if (lens < self.T0).any():
            raise ValueError("a slot's cache length cannot be below the shared prefix")
        dev = self.lens.device
        self.lens[torch.from_numpy(slots).to(dev)] = torch.from_numpy(lens.astype(np.int32)).to(dev)
        self.lens_host[slots] = lens

    def advance(self, n: int = 1) -> None:
        self.lens_host += int(n)

    def advance_rows(self, counts) -> None:
        """:meth:`advance` with one count per slot (a chunked decode step moves a slot by the tokens it fed)."""
        self.lens_host += np.asarray(counts, dtype=np.int64).reshape(self.B)

    def steps_reserved(self, slots) -> int:
        """Decode steps every slot in ``slots`` can still take within its pages."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if slots.size == 0:
            return 1 << 30
        return int((self.T0 + PAGE_ROWS * self.nch[slots] - self.lens_host[slots]).min())

    def compact(self, keep) -> None:
        """Keep only the slots ``keep`` (in that order) as rows 0..len(keep)-1; the other slots must have been
        released.  Page tables move with their rows, holds of shared contexts with them: no page is copied."""
        keep = np.asarray(keep, dtype=np.int64).reshape(-1)
        gone = np.setdiff1d(np.arange(self.B), keep)
        if gone.size and self.nch[gone].any():
            raise RuntimeError("compact: a dropped slot still holds pages")
        kt = torch.from_numpy(keep).to(self.table.device)
        self.table = self.table.index_select(0, kt).contiguous()
        self.lens = self.lens.index_select(0, kt).contiguous()
        self.host, self.nch, self.lens_host = self.host[keep], self.nch[keep], self.lens_host[keep]
        self.nshared = self.nshared[keep]
        self.slot_entry = [self.slot_entry[i] for i in keep.tolist()]
        self.slot_prefix = [self.slot_prefix[i] for i in keep.tolist()]
        self.B = int(keep.size)
        self.version += 1
