"""Slot schedulers of the native encode / decode loops (round 6): slot refill, page mapping, eviction, compaction.

The reference encodes every message in its own loop with its own KV cache (``code_base/arithmetic.py:96-122``; the
api splits a secret into independent chunks, ``src/neuralstego/api.py:736-747``).  Batched on the GPU, B messages
share one decode step; covers differ in length (a peaked, trained-LM-like row gives far longer covers than the
mean), so a lockstep batch spends its steps on finished streams.  Here messages queue for S SLOTS:

* every slot runs one message from the shared context (cache length ``T0``, the prefill's logits as its first
  coder step's row) to its end, with its own cache length and position ids (``lens[b] % n_positions``,
  ``code_base/arithmetic.py:44-48``) and its own KV pages (``lm/kvpages.py``);
* every ``check_every`` steps the host reads the coder states once: finished slots hand their tokens (or bits) over
  and take the next queued message; pages are mapped ahead for the live slots;
* when the device runs out of pages, the youngest live messages are EVICTED (pages returned, message re-queued and
  later re-run from its start -- the same tokens, since a stream's result does not depend on its neighbours) rather
  than failing; a message that cannot fit alone raises :class:`KVCapacityError`;
* when the queue is empty and at most half the slots are live, the live slots are COMPACTED into a smaller batch
  (page tables move with their rows, no KV is copied): the GEMMs stop computing finished rows.

With ``contexts`` (one per message, library 0.29) there is no shared context: a slot starts at cache length 0, an
admission maps the pages of each admitted message's own context plus its next steps, prefills those contexts ragged
into the pages (``BatchedGPT2.prefill_contexts``, at the host check, outside the step graph) and puts each context's
logits into its slot's row; an evicted message is prefilled again when it comes back.  Messages of the call that
carry the same context (library 0.30) share its full KV pages: the context is prefilled once while any of them holds
it, a holder maps only the pages after the context's full ones, and an evicted holder gives back only those.

A stream's logits are bit-identical whatever the batch it runs in (the decode step is batch-invariant, including the
paged attention), so a message's tokens are the same alone, in lockstep, or refilled into any slot.  Between host
checks the step (coder + GPT-2 decode) is one captured hipGraph replay; a graph is re-captured when a buffer it
holds is replaced (a wider page table, a longer history, a compaction).

With ``qualities`` (one coder quality per message, library 0.31) every slot also has a row of the coder's stream
quality table (``ns_set_stream_quality``): an admission -- the first fill, a refill, a re-admission after an eviction,
with or without per-message contexts -- writes the message's row together with its payload and fresh state, a
compaction permutes the table with the other per-slot tensors, and the table is part of the graph's layout key.

The rank coder (library 0.31.5) runs through the same loops: :class:`RankSlotEncoder` is :class:`SlotEncoder` over
``coder.RankStreamEncodeSession`` and :class:`RankSlotDecoder` is :class:`SlotSampler`'s loop over
``coder.RankStreamDecodeSession``, every slot with its message's row of the rank quality table
(``ns_rank_stream_quality``: temperature and policy), given to ``ns_rank_*_step_streams`` with each step.

The reveal from cover text (library 0.31.6) is :class:`SlotRevealer`, :class:`SlotSampler`'s loop over
``coder.DecodeStreamsSession`` (``ns_decode_step_streams``) with one difference: a stream's end is not known in
advance -- a span ends where its packet's JSON closes -- so every check asks ``cover._span_end`` about every live
slot, and what is left of a text after a settled span is queued as a fresh stream.
"""

from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence

import numpy as np

from .. import _lib
from ..coder import EncodeSession, _state_fields, _stats_rows
from ..exceptions import KVCapacityError


MAX_CHUNK = 16  # tokens of a stream per forward: ns_decode_attention_paged_chunk's limit


def check_chunk(chunk) -> int:
    """``chunk`` (known tokens of a stream per LM forward) as an int in 1..16, else ``ValueError``."""
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)):
        raise ValueError(f"chunk must be an int in 1..{MAX_CHUNK}, got {chunk!r}")
    if not 1 <= int(chunk) <= MAX_CHUNK:
        raise ValueError(f"chunk must be in 1..{MAX_CHUNK}, got {chunk}")
    return int(chunk)


def chunk_slots(n_messages: int, slots: int, chunk: int) -> int:
    """Slots of a decode that feeds ``chunk`` tokens per stream and forward: ``min(N, max(1, slots // chunk))``, so a
    forward has at most ``slots`` rows -- the activations and the logits take no more memory than the caller sized
    ``slots`` for (``chunk = 1``: ``min(N, slots)``, at least one)."""
    return max(1, min(int(n_messages), max(1, int(slots) // int(chunk))))


def chunk_counts(fed, nlen, chunk: int) -> np.ndarray:
    """Tokens each slot takes in the next chunked iteration: ``min(chunk, remaining)`` with ``remaining = nlen - fed``
    (never negative: a finished or empty slot takes none)."""
    return np.clip(np.asarray(nlen, dtype=np.int64) - np.asarray(fed, dtype=np.int64), 0, int(chunk))


def chunk_page_horizon(lens, ends, check_every: int, chunk: int) -> np.ndarray:
    """Positions below which a live slot needs pages until the next host check has mapped more: the next
    ``(check_every + 1) * chunk`` positions, capped at the message's end (``ends`` = context + token count)."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.minimum(lens + (int(check_every) + 1) * int(chunk), np.asarray(ends, dtype=np.int64))


class _SlotGraph:
    """``body()`` (one whole step into fixed buffers) run once eagerly on a side stream -- a real step, which also
    warms every kernel up -- then captured as a hipGraph and replayed per later step."""

    def __init__(self, body):
        import torch

        self.body = body
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()

    def replay(self) -> None:
        self.graph.replay()


def _layout_key(*tensors) -> tuple:
    return tuple(t.data_ptr() if t is not None else 0 for t in tensors)


class _Pinned:
    """Double-buffered pinned host copies of a device tensor, taken asynchronously on the current stream with an
    event (the check pipeline of the slot loops: a check reads the PREVIOUS check's copy, whose event the GPU has
    passed, while the steps enqueued since keep it busy)."""

    def __init__(self):
        self.bufs = [None, None]
        self.k = 0

    def take(self, dev_tensor):
        import torch

        b = self.bufs[self.k]
        if b is None or b.shape != dev_tensor.shape or b.dtype != dev_tensor.dtype:
            b = self.bufs[self.k] = torch.empty(dev_tensor.shape, dtype=dev_tensor.dtype, pin_memory=True)
        b.copy_(dev_tensor, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.k ^= 1
        return b, ev


def _rows_after(event, side, tensor, rows, ncols=None):
    """``tensor[rows, :ncols]`` on the host, gathered on the ``side`` stream once ``event`` has passed (rows that no
    later step writes: finished streams), without waiting for the steps enqueued on the main stream since."""
    import torch

    with torch.cuda.stream(side):
        side.wait_event(event)
        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=tensor.device)
        out = tensor.index_select(0, idx)
        if ncols is not None:
            out = out[:, :ncols]
        host = out.cpu()
    return host


def _trimmed(contexts, n: int) -> List[List[int]]:
    """One context per message, each trimmed to its last 1,022 ids as the shared prefill trims its one."""
    ctxs = [[int(t) for t in list(c)[-1022:]] for c in contexts]
    if len(ctxs) != n:
        raise ValueError(f"{len(ctxs)} contexts for {n} messages")
    if any(len(c) < 1 for c in ctxs):
        raise ValueError("context must contain at least one token")
    return ctxs


def _multiplicity(contexts, share: bool):
    """``(keys, shares)`` of a call's trimmed contexts: whether the message shares its context's pages -- more than
    one message of the whole call carries it -- and then the context as a tuple, the key of its entry (else None)."""
    from .kvpages import sharing_keys

    keys = sharing_keys(contexts) if share else [None] * len(contexts)
    return keys, [k is not None for k in keys]


def _prefix_chains(contexts, on: bool):
    """One chain of shared prefix runs per message (``kvpages.plan_prefixes`` over the whole call's trimmed contexts:
    a prefix counts when at least two distinct contexts of the CALL begin with it), or None when prefixes are not
    shared."""
    from .kvpages import plan_prefixes

    chains = plan_prefixes(contexts) if on else None
    return chains if chains is not None and any(chains) else None


def _admissible(queue, contexts, check_every: int, nslots: int, room: int, keys=None, shares=None,
                live=(), chains=None, live_prefixes=()) -> List[int]:
    """Pop the messages to admit now from the queue's front: at most ``nslots``, while the pages of their contexts
    and first ``check_every + 1`` positions fit in ``room`` pages (what the pool can still hand out beyond one page
    per live slot).  The admission then maps exactly these pages.  A message that shares its context
    (``shares[m]``, entry key ``keys[m]``) counts its own pages only -- those after the context's full pages -- and
    its entry's pages once, with the first message of this batch that opens it, unless the entry is ``live``.  A
    message with a chain of shared prefix runs (``chains[m]``) counts the pages after the chain only, and each run's
    pages once in the same way, unless the run is in ``live_prefixes``; a live entry's chain is live with it."""
    from .kvpages import chain_past, own_pages, shared_pages

    out, used, opened, popened = [], 0, set(), set()
    while queue and len(out) < nslots:
        m = queue[0]
        T = len(contexts[m])
        sh = shares is not None and shares[m]
        chain = chains[m] if chains is not None else ()
        past = chain_past(chain)
        need = own_pages(T, check_every + 1, sh, past)
        opens = sh and keys[m] not in live and keys[m] not in opened
        if opens:
            need += shared_pages(T, past)
        runs = [k for k, a, b in chain if k not in live_prefixes and k not in popened] if opens or not sh else []
        need += sum(shared_pages(b, a) for k, a, b in chain if k in runs)
        if used + need > room:
            break
        used += need
        if opens:
            opened.add(keys[m])
        popened.update(runs)
        out.append(queue.popleft())
    return out


def _map_contexts(kv, slots, keys, shares, tl, upto, chains=None) -> np.ndarray:
    """Page mapping of an admission with per-message contexts: every slot in ``slots`` starts over at its context's
    length ``tl``, a sharing message holds its context's entry (opened here if it is not live), and every message
    gets its own pages for the positions below ``upto``.  A message with a chain of shared prefix runs (``chains``,
    one per slot) holds the chain too -- beneath its context's entry, or itself when only the prefix is shared.
    Returns the mask of the slots that were served; the others are left released (the pool is out of memory)."""
    kv.reset(slots, lens=tl)
    sh = np.asarray(shares, dtype=bool)
    failed = set()
    if chains is not None:
        hd = sh | np.asarray([bool(c) for c in chains], dtype=bool)
        if hd.any():
            failed = set(kv.hold(slots[hd], [k if f else None for k, f, h in zip(keys, sh, hd) if h], tl[hd],
                                 [c for c, h in zip(chains, hd) if h]).tolist())
    elif sh.any():
        failed = set(kv.hold(slots[sh], [k for k, f in zip(keys, sh) if f], tl[sh]).tolist())
    rest = np.asarray([s not in failed for s in slots.tolist()], dtype=bool)
    failed |= set(kv.ensure(slots[rest], upto[rest]).tolist())
    ok = np.asarray([s not in failed for s in slots.tolist()], dtype=bool)
    if not ok.all():
        kv.reset(slots[~ok])
    return ok


class SlotEncoder:
    """Encode ``bit_lists`` through ``slots`` slots of ``provider.lm`` (a native :class:`BatchedGPT2`)."""

    def __init__(self, provider, ctx, bit_lists: Sequence[Sequence[int]], context: Sequence[int], *, slots: int,
                 finish: bool, stop_text: Optional[str], stats: bool, check_every: int, stall_steps: int,
                 hard_cap: int, use_graph: bool, compact: bool = True,
                 contexts: Optional[Sequence[Sequence[int]]] = None, share: bool = True, qualities=None,
                 share_prefixes: bool = True):
        self.p, self.lm, self.ctx = provider, provider.lm, ctx
        self.qual = qualities  # coder.StreamQuality with one row per message, or None (the context's one quality)
        self.bits = bit_lists
        self.N = len(bit_lists)
        self.S = max(1, min(int(slots), self.N))
        self.context = context
        # one context per message (``context`` is then None): every admission prefills the admitted messages'
        # contexts into their slots' own pages (``BatchedGPT2.prefill_contexts``), no shared prefix
        self.contexts = _trimmed(contexts, self.N) if contexts is not None else None
        # messages of the call with equal contexts share the context's KV pages (lm/kvpages.py)
        self.keys, self.shares = _multiplicity(self.contexts, share) if contexts is not None else (None, None)
        # different contexts of the call share the pages of a common prefix (fp16 pages only: lm.prefix_sharing)
        self.chains = _prefix_chains(self.contexts, share and share_prefixes and
                                     getattr(self.lm, "prefix_sharing", False)) if contexts is not None else None
        self.prefix_rows_saved = self.prefix_entries = 0
        self.prefill_shared = 0
        self.ctx_len = np.zeros(self.S, dtype=np.int64)  # context rows of the message in each slot (per-context)
        self.prefill_rows = 0
        self.prefill_groups = 0
        self.finish, self.stop_text, self.stats = finish, stop_text, stats
        self.check_every, self.stall_steps, self.hard_cap = int(check_every), int(stall_steps), int(hard_cap)
        self.use_graph, self.allow_compact = use_graph, compact
        self.evictions = 0
        self.compactions = 0
        self.max_live = 0
        self.kv_peak = 0

    # ------------------------------------------------------------------
    def run(self):
        import torch

        from ..codec.errors import ArithmeticRangeError
        from .arithmetic import _StopCheck

        lm, S, N = self.lm, self.S, self.N
        max_bits = max(len(b) for b in self.bits)
        # initial token-history / page-table width (both grow on demand; a provider may set a small one in tests)
        budget = getattr(self.p, "slot_budget_tokens", None) or 2 * max_bits + 64
        per_ctx = self.contexts is not None
        if per_ctx:  # no shared prefix: every slot starts empty and the first check admits from the queue
            lm.begin_slots(S, 0, budget)
            logits = torch.zeros((S, lm.ld), device=lm.device, dtype=lm.logits_dtype)
            first = None
        else:
            logits = lm.prefill(self.context, S, budget)  # [S, ld]: every slot starts on the context's logits
            first = lm.first_logits
        T0 = lm.kv.T0
        stride = max(1, (max_bits + 7) // 8)
        sess = self._session(S, budget, stride)
        stop = _StopCheck(self.p, sess, self.stop_text) if self.stop_text is not None else None
        if per_ctx:
            sess.park_slots(np.arange(S))
            slot_msg = np.full(S, -1, dtype=np.int64)
            queue = deque(range(N))
        else:
            slot_msg = np.arange(S, dtype=np.int64)  # message per slot, -1 = empty
            queue = deque(range(S, N))
        tokens: List[Optional[List[int]]] = [None] * N
        stats_out: List[Optional[dict]] = [None] * N
        last_pos = np.zeros(S, dtype=np.int64)
        last_move = np.zeros(S, dtype=np.int64)
        t = 0
        graph, gkey = None, None
        admit_blocked = False

        def body():
            tok = sess.step(logits, finish_sent=self.finish)
            if stop is not None:
                stop.flag(tok)
            lm.step_static(tok)

        skip = getattr(self.p, "skip_done", True)  # finished streams skip their attention (A/B switch)

        def done_view():
            return sess.state.view(torch.int32)[:, 7] if skip else None

        # check pipeline (graph replays, no per-step stop test): a check processes the coder states copied at the
        # PREVIOUS check while the steps enqueued since run -- the GPU never waits for the host; a finished slot is
        # seen one period later (it idles through it, skipping its attention) and its tokens are gathered on a side
        # stream.  Eager or stop-text loops read the states synchronously.
        pipelined = self.use_graph and stop is None
        pin, pending = _Pinned(), None
        side = torch.cuda.Stream() if pipelined else None
        lm.begin_static(logits)
        lm.done_flags = done_view()
        try:
            while True:
                if stop is not None and t > 0:
                    stop.check()
                if t % self.check_every == 0:
                    if pipelined:
                        f, ev = (None, None) if pending is None else (pending[0], pending[1])
                        if ev is not None:
                            ev.synchronize()
                            f = _state_fields(f)
                    else:
                        f, ev = sess.fields(), None
                    live = slot_msg >= 0
                    flags = f["flags"] if f is not None else np.zeros(sess.B, dtype=np.uint32)
                    # ---- harvest finished slots
                    fin = np.nonzero(live & ((flags & _lib.NS_ST_DONE) != 0))[0]
                    if fin.size:
                        bad = fin[(flags[fin] & _lib.NS_ST_ERR_RANGE) != 0]
                        if bad.size:
                            raise ArithmeticRangeError(self._range_error(slot_msg[bad].tolist()[:8]))
                        nt = f["ntokens"][fin]
                        if int(nt.max(initial=0)) > sess.hist.shape[1]:
                            raise RuntimeError("token history overflow")
                        ncol = max(1, int(nt.max()))
                        if ev is not None:
                            host = _rows_after(ev, side, sess.hist, fin, ncol).numpy()
                            acc = _rows_after(ev, side, sess.stats_acc, fin).numpy() if self.stats else None
                        else:
                            host = sess.hist[torch.as_tensor(fin, device=sess.hist.device), :ncol].cpu().numpy()
                            acc = sess.stats_acc[torch.as_tensor(fin, device=sess.hist.device)].cpu().numpy() \
                                if self.stats else None
                        for j, s in enumerate(fin.tolist()):
                            m = int(slot_msg[s])
                            tokens[m] = host[j, : int(nt[j])].tolist()
                            if self.stats:
                                stats_out[m] = _stats_rows(acc[j:j + 1], f["bit_pos"][s:s + 1])[0]
                        self._harvested(sess, fin, slot_msg[fin], nt, ev, side)
                        lm.kv.release(fin)
                        slot_msg[fin] = -1
                        admit_blocked = False
                        live = slot_msg >= 0
                    # ---- stalls (the reference loops forever on a stream that fixes no bit)
                    pos = f["bit_pos"] if f is not None else last_pos
                    ntok = f["ntokens"] if f is not None else np.zeros(sess.B, dtype=np.int64)
                    moved = live & (pos != last_pos)
                    last_pos[moved], last_move[moved] = pos[moved], t
                    stuck = np.nonzero(live & (((t - last_move) >= self.stall_steps) |
                                               (ntok >= self.hard_cap)))[0]
                    if stuck.size:
                        ids = slot_msg[stuck].tolist()[:8]
                        if all(pos[s] >= len(self.bits[slot_msg[s]]) for s in stuck):
                            raise ArithmeticRangeError(
                                f"finish_sent: streams {ids} produced no sentence-ending token in "
                                f"{self.stall_steps} tokens (the reference would keep generating forever)")
                        raise ArithmeticRangeError(
                            f"streams {ids} fixed no payload bit for {self.stall_steps} tokens: the interval "
                            "straddles the midpoint and one token takes the whole range (the reference coder "
                            "has no underflow handling and would loop forever)")
                    # ---- refill empty slots from the queue
                    empty = np.nonzero(~live)[0]
                    if queue and empty.size and not admit_blocked:
                        room = lm.pool.free_pages + lm.pool.growable_pages() - int(live.sum()) - 1
                        if per_ctx:
                            ms = _admissible(queue, self.contexts, self.check_every, empty.size, room, self.keys,
                                             self.shares, lm.kv.entries, self.chains, lm.kv.prefixes)
                            if ms:
                                back = self._admit_contexts(sess, logits, empty[:len(ms)], ms, slot_msg, last_pos,
                                                            last_move, t)
                                queue.extendleft(reversed(back))
                                admit_blocked = bool(back)
                                live = slot_msg >= 0
                        else:
                            n_adm = int(min(empty.size, len(queue), max(0, room)))
                            if n_adm:
                                sl = empty[:n_adm]
                                ms = [queue.popleft() for _ in range(n_adm)]
                                self._admit(sess, logits, first, sl, ms, slot_msg, last_pos, last_move, t)
                                live = slot_msg >= 0
                    nlive = int(live.sum())
                    self.max_live = max(self.max_live, nlive)
                    if nlive == 0:
                        if not queue:
                            break
                        if per_ctx:
                            m = queue[0]
                            raise KVCapacityError(
                                f"message {m}: no device memory for the KV pages of its {len(self.contexts[m])}-token "
                                f"context ({lm.pool.total} pages of {lm.pool.page_bytes} B)")
                        raise KVCapacityError("no device memory for even one stream's first KV page")
                    # ---- compaction: the queue is drained and at most half the slots are live
                    compacted = False
                    if self.allow_compact and not queue and nlive <= sess.B // 2 and sess.B > 1:
                        compacted = True
                        if f is not None:
                            ntok = ntok[np.nonzero(live)[0]]
                        keep = np.nonzero(live)[0]
                        sess, logits, slot_msg, last_pos, last_move = self._compact(
                            sess, logits, keep, slot_msg, last_pos, last_move, stop)
                        self.ctx_len = self.ctx_len[keep].copy()
                        if stop is not None:
                            stop.sess = sess
                            stop.hit = torch.zeros(sess.B, dtype=torch.bool, device=sess.state.device)
                        live = slot_msg >= 0
                        self.compactions += 1
                    # ---- pages for the next check_every + 1 steps; evict the youngest when the device is full
                    self._map_pages(sess, slot_msg, queue, live, T0)
                    if (slot_msg >= 0).sum() < nlive:
                        admit_blocked = True
                    # ---- token history for the next steps (two periods ahead of a pipelined state copy)
                    ahead = (2 if pipelined else 1) * self.check_every + 1
                    if int(ntok.max(initial=0)) + ahead > sess.hist.shape[1]:
                        sess.ensure_history(ahead)
                    if stop is not None:
                        stop.sess = sess
                    if pipelined:
                        pending = pin.take(sess.state)
                key = _layout_key(logits, sess.state, sess.hist, sess.payload, lm.kv.table, lm.kv.lens,
                                  sess.stats_acc, sess.qtable) + (lm.kv.version,) + self._key_extra(sess)
                if self.use_graph:
                    if graph is None or key != gkey:
                        graph = None
                        lm.done_flags = done_view()
                        lm.begin_static(logits)
                        graph, gkey = _SlotGraph(body), key
                    else:
                        graph.replay()
                else:
                    lm.done_flags = done_view()
                    lm.begin_static(logits)
                    body()
                lm.advance(1)
                t += 1
        finally:
            if graph is not None:  # a pipelined loop ends with steps still queued on its graph
                torch.cuda.current_stream().synchronize()
            lm.done_flags = None
            del graph
        self.sess = sess
        self.kv_peak = lm.kv.peak
        return tokens, (stats_out if self.stats else None)

    # ------------------------------------------------------------------
    def _rows(self, msgs):
        """The quality rows of messages ``msgs`` (None without per-message qualities)."""
        return self.qual.take(list(msgs)) if self.qual is not None else None

    # what a subclass with another coder session replaces (RankSlotEncoder)
    def _session(self, S: int, budget: int, stride: int):
        """The coder session of the run: the first S messages loaded (a per-context run parks them all first)."""
        return EncodeSession(self.ctx, self.bits[:S], max_tokens=budget, stats=self.stats, payload_stride=stride,
                             quality=self._rows(range(S)))

    def _range_error(self, msgs) -> str:
        return f"streams {msgs} found no CDF bucket for the payload index"

    def _harvested(self, sess, fin, msgs, nt, ev, side) -> None:
        """Finished slots ``fin`` (messages ``msgs``, ``nt`` tokens each) just handed their tokens over."""

    def _key_extra(self, sess) -> tuple:
        return ()

    def _admit(self, sess, logits, first, slots, msgs, slot_msg, last_pos, last_move, t):
        import torch

        lm = self.lm
        sess.load_slots(slots, [self.bits[m] for m in msgs], quality=self._rows(msgs))
        lm.kv.reset(slots)
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=logits.device)
        logits.index_copy_(0, idx, first.expand(len(slots), -1).to(logits.dtype))
        slot_msg[slots] = msgs
        last_pos[slots] = 0
        last_move[slots] = t

    def _admit_contexts(self, sess, logits, slots, msgs, slot_msg, last_pos, last_move, t):
        """Admit ``msgs`` with their own contexts into ``slots``: pages for each context and the next
        ``check_every + 1`` positions, one ragged prefill of the contexts into those pages, the first logits into the
        slots' rows.  Returns the messages that could not be given pages (back to the queue, in order)."""
        import torch

        lm = self.lm
        slots = np.asarray(slots, dtype=np.int64)
        tl = np.asarray([len(self.contexts[m]) for m in msgs], dtype=np.int64)
        chains = [self.chains[m] for m in msgs] if self.chains is not None else None
        ok = _map_contexts(lm.kv, slots, [self.keys[m] for m in msgs], [self.shares[m] for m in msgs], tl,
                           tl + self.check_every + 1, chains)
        back = [m for m, k in zip(msgs, ok) if not k]
        slots, msgs = slots[ok], [m for m, k in zip(msgs, ok) if k]
        if not msgs:
            return back
        first = lm.prefill_contexts([self.contexts[m] for m in msgs], slots, [self.shares[m] for m in msgs],
                                    [self.chains[m] for m in msgs] if self.chains is not None else None)
        self.prefix_rows_saved += lm.last_prefill.get("prefix_rows_saved", 0)
        self.prefix_entries += lm.last_prefill.get("prefix_entries", 0)
        self.prefill_rows += lm.last_prefill["rows"]
        self.prefill_groups += lm.last_prefill["groups"]
        self.prefill_shared += lm.last_prefill["shared"]
        sess.load_slots(slots, [self.bits[m] for m in msgs], quality=self._rows(msgs))
        idx = torch.as_tensor(slots, device=logits.device)
        logits.index_copy_(0, idx, first.to(logits.dtype))
        slot_msg[slots] = msgs
        self.ctx_len[slots] = tl[ok]
        last_pos[slots] = 0
        last_move[slots] = t
        return back

    def _map_pages(self, sess, slot_msg, queue, live, T0):
        """Pages for every live slot's next ``check_every + 1`` positions; on a full device evict the youngest live
        messages (fewest positions fed) back to the queue's front until the others are served."""
        lm = self.lm
        while True:
            sl = np.nonzero(slot_msg >= 0)[0]
            if sl.size == 0:
                return
            failed = lm.kv.ensure(sl, lm.kv.lens_host[sl] + self.check_every + 1)
            if failed.size == 0:
                return
            if sl.size == 1:
                raise KVCapacityError(
                    f"message {int(slot_msg[sl[0]])} needs more KV pages than the device holds "
                    f"({lm.pool.total} pages of {lm.pool.page_bytes} B)")
            # the youngest: fewest positions fed (its own context's rows, prefilled again later, do not count)
            victim = np.asarray([sl[np.argmin(lm.kv.lens_host[sl] - self.ctx_len[sl])]])
            queue.appendleft(int(slot_msg[victim[0]]))
            lm.kv.release(victim)
            sess.park_slots(victim)
            slot_msg[victim] = -1
            self.evictions += 1

    def _compact(self, sess, logits, keep, slot_msg, last_pos, last_move, stop):
        import torch

        lm = self.lm
        empty = np.setdiff1d(np.arange(sess.B), keep)
        lm.kv.release(empty)
        lm.kv.compact(keep)
        lm.B = lm.kv.B
        sess.compact(keep)
        idx = torch.as_tensor(keep, device=logits.device)
        logits = logits.index_select(0, idx).contiguous()
        return sess, logits, slot_msg[keep].copy(), last_pos[keep].copy(), last_move[keep].copy()


class SlotDecoder:
    """Decode ``token_lists`` through ``slots`` slots, longest first: pages are mapped as the streams grow (as the
    encoder maps them, with the same eviction), and a slot's end is known on the host from its token count."""

    def __init__(self, provider, ctx, token_lists: Sequence[Sequence[int]], context: Sequence[int], *, slots: int,
                 use_graph: bool, check_every: int = 16, compact: bool = True,
                 contexts: Optional[Sequence[Sequence[int]]] = None, share: bool = True, qualities=None,
                 share_prefixes: bool = True, chunk: int = 1):
        self.p, self.lm, self.ctx = provider, provider.lm, ctx
        self.qual = qualities  # coder.StreamQuality with one row per message, or None
        self.lists = token_lists
        self.N = len(token_lists)
        # chunk = C > 1: every iteration feeds a slot's next C known tokens in one forward (run_chunk), through
        # min(N, max(1, slots // C)) slots -- a forward then has at most ``slots`` rows
        self.C = check_chunk(chunk)
        if self.C > 1:
            if not getattr(self.lm, "native", False):
                raise ValueError("chunk > 1 needs the native HIP step")
            if getattr(self.lm, "window", 0) > 0:
                raise ValueError("chunk > 1 does not support a sliding attention window")
        self.S = chunk_slots(self.N, slots, self.C)
        self.context = context
        self.contexts = _trimmed(contexts, self.N) if contexts is not None else None  # one per message
        self.keys, self.shares = _multiplicity(self.contexts, share) if contexts is not None else (None, None)
        # different contexts of the call share the pages of a common prefix (fp16 pages only: lm.prefix_sharing)
        self.chains = _prefix_chains(self.contexts, share and share_prefixes and
                                     getattr(self.lm, "prefix_sharing", False)) if contexts is not None else None
        self.prefix_rows_saved = self.prefix_entries = 0
        self.prefill_shared = 0
        self.prefill_rows = 0
        self.prefill_groups = 0
        self.use_graph, self.check_every, self.allow_compact = use_graph, int(check_every), compact
        self.ahead = (self.check_every + 1) * self.C  # positions mapped ahead of a host check
        self.compactions = 0
        self.evictions = 0

    def run(self) -> List[List[int]]:
        import torch

        if self.C > 1:
            return self.run_chunk()

        from .. import _lib as L
        from ..codec.errors import DecodeDivergenceError
        from ..coder import _bit_rows_to_lists, _ptr, _state_tensor, _stream_handle, _table_registered

        lm, S, N = self.lm, self.S, self.N
        lens_all = np.asarray([len(t) for t in self.lists], dtype=np.int64)
        Tcap = max(1, int(lens_all.max(initial=0)))
        order = np.argsort(-lens_all, kind="stable")  # longest first: the tail is short messages
        per_ctx = self.contexts is not None
        if per_ctx:  # no shared prefix: a message's context is prefilled into its slot's pages at admission
            lm.begin_slots(S, 0, Tcap + 1)
            logits = torch.zeros((S, lm.ld), device=lm.device, dtype=lm.logits_dtype)
            first = None
        else:
            logits = lm.prefill(self.context, S, Tcap + 1)
            first = lm.first_logits
        T0 = lm.kv.T0
        dev = logits.device
        qual = self.qual
        P = qual.max_precision if qual is not None else self.ctx.params.precision  # the call's largest
        out_stride = int((Tcap * P + P + 7) // 8 + 8)
        st = {"tokmat": torch.zeros((S, Tcap), dtype=torch.int32, device=dev),
              "nlen": torch.zeros(S, dtype=torch.int32, device=dev),
              "stop": torch.zeros(S, dtype=torch.int32, device=dev),
              "state": _state_tensor(S, dev),
              "out_bits": torch.zeros((S, out_stride), dtype=torch.uint8, device=dev)}
        if per_ctx:  # context rows of the message in each slot: the token index is lens - ctx (moves with compaction)
            st["ctx"] = torch.zeros(S, dtype=torch.int32, device=dev)
        if qual is not None:  # the slots' quality rows (moves with compaction; every slot starts parked on a valid row)
            st["quality"] = qual.take([0] * S).table(dev)
        ctx_host = np.full(S, T0, dtype=np.int64)
        self.ctx.check(L.lib().ns_init_state(self.ctx._h, _ptr(st["state"]), S, _stream_handle()), "ns_init_state")
        st["state"].view(torch.int32)[:, 7] = L.NS_ST_DONE
        slot_msg = np.full(S, -1, dtype=np.int64)
        nlen_host = np.zeros(S, dtype=np.int64)
        queue = deque(order.tolist())
        out: List[Optional[List[int]]] = [None] * N
        init_row = torch.tensor([[0, 1 << P, 0, 0]], dtype=torch.int64, device=dev)
        p = self.ctx.params
        k_max = qual.k_max if qual is not None else 0
        graph, gkey = None, None
        bufs = {}
        admit_blocked = False

        def body():
            tix = lm.kv.lens - (st["ctx"] if per_ctx else T0)
            idx = tix.clamp(0, Tcap - 1).long().unsqueeze(1)
            tok = torch.gather(st["tokmat"], 1, idx).squeeze(1).contiguous()
            act = (tix < st["nlen"]).to(torch.uint8)
            last = (tix == st["nlen"] - 1).to(torch.uint8)
            bufs["tok"], bufs["act"], bufs["last"] = tok, act, last
            with _table_registered(self.ctx, st.get("quality"), k_max):
                rc = L.lib().ns_decode_step(self.ctx._h, _ptr(logits), logits.stride(0), st["state"].shape[0],
                                            _ptr(tok), _ptr(last), _ptr(act), _ptr(st["state"]), _ptr(st["out_bits"]),
                                            out_stride, float(p.temp), int(p.topk), self.ctx._banned,
                                            self.ctx._nbanned, None, 0, _stream_handle())
            self.ctx.check(rc, "ns_decode_step")
            lm.step_static(tok)

        t = 0
        # check pipeline as in the encoder: a slot counts as finished once the event recorded at the previous check
        # has passed with its last token fed (its message and positions as of that check); its bits are gathered on a
        # side stream while the steps enqueued since run
        pipelined = self.use_graph
        side = torch.cuda.Stream() if pipelined else None
        pending = None
        try:
            while True:
                if t % self.check_every == 0:
                    live = slot_msg >= 0
                    if pipelined:
                        if pending is not None:
                            ev, msg_then, fed_then = pending
                            ev.synchronize()
                            done = live & (slot_msg == msg_then) & (fed_then >= nlen_host)
                        else:
                            ev, done = None, np.zeros(slot_msg.shape, dtype=bool)
                    else:
                        ev, done = None, live & ((lm.kv.lens_host - ctx_host) >= nlen_host)
                    fin = np.nonzero(done)[0]
                    if fin.size:
                        if ev is not None:
                            srows = _rows_after(ev, side, st["state"], fin).numpy()
                            f = _state_fields(torch.from_numpy(srows))
                            rows = _rows_after(ev, side, st["out_bits"], fin)
                        else:
                            f = _state_fields(st["state"][torch.as_tensor(fin, device=dev)])
                            rows = st["out_bits"][torch.as_tensor(fin, device=dev)]
                        bad = fin[(f["flags"] & L.NS_ST_ERR_DIVERGE) != 0]
                        if bad.size:
                            raise DecodeDivergenceError(
                                f"streams {slot_msg[bad].tolist()[:8]}: received token outside the kept top-k")
                        got = _bit_rows_to_lists(rows, f["bit_pos"])
                        for j, s in enumerate(fin.tolist()):
                            out[int(slot_msg[s])] = got[j]
                        lm.kv.release(fin)
                        slot_msg[fin] = -1
                        nlen_host[fin] = 0
                        admit_blocked = False
                        fi = torch.as_tensor(fin, device=dev)
                        st["nlen"][fi] = 0
                        st["stop"][fi] = 0
                        live = slot_msg >= 0
                    empty = np.nonzero(~live)[0]
                    if queue and empty.size and not admit_blocked:
                        room = lm.pool.free_pages + lm.pool.growable_pages() - int(live.sum()) - 1
                        if per_ctx:
                            adm_m = _admissible(queue, self.contexts, self.check_every, empty.size, room,
                                                self.keys, self.shares, lm.kv.entries, self.chains,
                                                lm.kv.prefixes)
                            if adm_m:
                                back = self._admit_contexts(st, logits, init_row, empty[:len(adm_m)], adm_m, slot_msg,
                                                            nlen_host, ctx_host, Tcap)
                                queue.extendleft(reversed(back))
                                admit_blocked = bool(back)
                                live = slot_msg >= 0
                            if not live.any():
                                m = queue[0]
                                raise KVCapacityError(
                                    f"message {m}: no device memory for the KV pages of its "
                                    f"{len(self.contexts[m])}-token context")
                        else:
                            n_adm = int(min(empty.size, len(queue), max(0, room)))
                            if n_adm:
                                adm_s = empty[:n_adm]
                                adm_m = [queue.popleft() for _ in range(n_adm)]
                                lm.kv.reset(adm_s)
                                self._admit(st, logits, first, init_row, adm_s, adm_m, slot_msg, nlen_host, T0, Tcap)
                                live = slot_msg >= 0
                    # pages for the next check_every + 1 positions (never past a message's last fed token); on a full
                    # device the youngest messages go back to the queue's front (re-decoded later: the same bits)
                    while live.any():
                        sl = np.nonzero(live)[0]
                        upto = np.minimum(lm.kv.lens_host[sl] + self.check_every + 1, ctx_host[sl] + nlen_host[sl])
                        if lm.kv.ensure(sl, upto).size == 0:
                            break
                        if sl.size == 1:
                            raise KVCapacityError(f"message {int(slot_msg[sl[0]])} ({int(nlen_host[sl[0]])} tokens) "
                                                  "needs more KV pages than the device holds")
                        v = sl[np.argmin(lm.kv.lens_host[sl] - ctx_host[sl])]  # the youngest: fewest tokens fed
                        queue.appendleft(int(slot_msg[v]))
                        lm.kv.release([v])
                        vi = torch.as_tensor([int(v)], device=dev)
                        st["nlen"][vi] = 0
                        st["stop"][vi] = 0
                        slot_msg[v], nlen_host[v] = -1, 0
                        live = slot_msg >= 0
                        admit_blocked = True
                        self.evictions += 1
                    if not live.any():
                        break
                    if self.allow_compact and not queue and int(live.sum()) <= st["state"].shape[0] // 2 and \
                            st["state"].shape[0] > 1:
                        keep = np.nonzero(live)[0]
                        lm.kv.release(np.setdiff1d(np.arange(st["state"].shape[0]), keep))
                        lm.kv.compact(keep)
                        lm.B = lm.kv.B
                        ki = torch.as_tensor(keep, device=dev)
                        for k in st:
                            st[k] = st[k].index_select(0, ki).contiguous()
                        logits = logits.index_select(0, ki).contiguous()
                        slot_msg, nlen_host = slot_msg[keep].copy(), nlen_host[keep].copy()
                        ctx_host = ctx_host[keep].copy()
                        self.compactions += 1
                    lm.stop_len = st["stop"] if getattr(self.p, "skip_done", True) else None
                    if pipelined:
                        ev_now = torch.cuda.Event()
                        ev_now.record()
                        pending = (ev_now, slot_msg.copy(), lm.kv.lens_host - ctx_host)
                key = _layout_key(logits, st["state"], st["tokmat"], lm.kv.table, lm.kv.lens, st.get("ctx"),
                                  st.get("quality")) + (lm.kv.version,)
                if self.use_graph:
                    if graph is None or key != gkey:
                        graph = None
                        lm.begin_static(logits)
                        graph, gkey = _SlotGraph(body), key
                    else:
                        graph.replay()
                else:
                    lm.begin_static(logits)
                    body()
                lm.advance(1)
                t += 1
        finally:
            if graph is not None:
                torch.cuda.current_stream().synchronize()
            lm.stop_len = None
            del graph
        return out

    def run_chunk(self) -> List[List[int]]:
        """:meth:`run` with ``C = chunk`` known tokens per slot and iteration.  The LM forward over a cover does not
        depend on the coder, so one iteration is: one forward over every live slot's next ``n = min(C, remaining)``
        tokens (``BatchedGPT2.step_chunk_static``: a slot's K/V pages are read once per C tokens; every logits row the
        bits of the one-token step), then C ``ns_decode_step`` launches -- launch i over the rows that predict each
        slot's token i, a slot active while i < n.  Launch 0 reads the ``carry`` row ([S, ld]: what the previous
        iteration, or the context prefill at admission, predicted), launch i > 0 row i - 1 of the forward's
        ``[S, C, ld]`` logits (slot stride C * ld); the forward's last row becomes the next carry.  The whole
        iteration is one captured graph body.  Admission, page mapping (``(check_every + 1) * C`` positions ahead),
        eviction, compaction and the per-message contexts, qualities and shared pages are those of :meth:`run`."""
        import torch

        from .. import _lib as L
        from ..codec.errors import DecodeDivergenceError
        from ..coder import _bit_rows_to_lists, _ptr, _state_tensor, _stream_handle, _table_registered

        lm, S, N, C = self.lm, self.S, self.N, self.C
        lens_all = np.asarray([len(t) for t in self.lists], dtype=np.int64)
        Tcap = max(1, int(lens_all.max(initial=0)))
        order = np.argsort(-lens_all, kind="stable")  # longest first: the tail is short messages
        per_ctx = self.contexts is not None
        if per_ctx:
            lm.begin_slots(S, 0, Tcap + 1)
            carry = torch.zeros((S, lm.ld), device=lm.device, dtype=lm.logits_dtype)
            first = None
        else:
            carry = lm.prefill(self.context, S, Tcap + 1)
            first = lm.first_logits
        T0 = lm.kv.T0
        dev = carry.device
        logits = torch.zeros((S, C, lm.ld), device=dev, dtype=lm.logits_dtype)
        qual = self.qual
        P = qual.max_precision if qual is not None else self.ctx.params.precision
        out_stride = int((Tcap * P + P + 7) // 8 + 8)
        st = {"tokmat": torch.zeros((S, Tcap), dtype=torch.int32, device=dev),
              "nlen": torch.zeros(S, dtype=torch.int32, device=dev),
              "stop": torch.zeros(S, dtype=torch.int32, device=dev),
              "state": _state_tensor(S, dev),
              "out_bits": torch.zeros((S, out_stride), dtype=torch.uint8, device=dev)}
        if per_ctx:
            st["ctx"] = torch.zeros(S, dtype=torch.int32, device=dev)
        if qual is not None:
            st["quality"] = qual.take([0] * S).table(dev)
        ctx_host = np.full(S, T0, dtype=np.int64)
        self.ctx.check(L.lib().ns_init_state(self.ctx._h, _ptr(st["state"]), S, _stream_handle()), "ns_init_state")
        st["state"].view(torch.int32)[:, 7] = L.NS_ST_DONE
        slot_msg = np.full(S, -1, dtype=np.int64)
        nlen_host = np.zeros(S, dtype=np.int64)
        queue = deque(order.tolist())
        out: List[Optional[List[int]]] = [None] * N
        init_row = torch.tensor([[0, 1 << P, 0, 0]], dtype=torch.int64, device=dev)
        p = self.ctx.params
        k_max = qual.k_max if qual is not None else 0
        graph, gkey = None, None
        bufs = {}
        admit_blocked = False
        ar = torch.arange(C, device=dev, dtype=torch.int32).unsqueeze(0)

        def body():
            tix = lm.kv.lens - (st["ctx"] if per_ctx else T0)  # tokens fed = the token the carry row predicts
            cnt = (st["nlen"] - tix).clamp(0, C)
            pos = tix.unsqueeze(1) + ar  # [S, C] token indices of the iteration
            tok = torch.gather(st["tokmat"], 1, pos.clamp(0, Tcap - 1).long()).contiguous()
            tokT = tok.t().contiguous()  # launch i's tokens, contiguous
            act = (ar < cnt.unsqueeze(1)).to(torch.uint8).t().contiguous()
            last = (pos == (st["nlen"] - 1).unsqueeze(1)).to(torch.uint8).t().contiguous()
            bufs["tok"], bufs["tokT"], bufs["act"], bufs["last"], bufs["cnt"] = tok, tokT, act, last, cnt
            lm.step_chunk_static(tok, cnt)  # lens += cnt
            ld_slot = logits.stride(0)
            with _table_registered(self.ctx, st.get("quality"), k_max):
                for i in range(C):
                    rows, ld = (carry, carry.stride(0)) if i == 0 else (logits[:, i - 1], ld_slot)
                    rc = L.lib().ns_decode_step(self.ctx._h, rows.data_ptr(), ld, st["state"].shape[0],
                                                _ptr(tokT[i]), _ptr(last[i]), _ptr(act[i]), _ptr(st["state"]),
                                                _ptr(st["out_bits"]), out_stride, float(p.temp), int(p.topk),
                                                self.ctx._banned, self.ctx._nbanned, None, 0, _stream_handle())
                    self.ctx.check(rc, "ns_decode_step")
            carry.copy_(logits[:, C - 1])  # a slot that fed fewer than C tokens has ended: its carry is not read

        t = 0
        pipelined = self.use_graph
        side = torch.cuda.Stream() if pipelined else None
        pending = None
        lm.stop_len = None
        try:
            while True:
                if t % self.check_every == 0:
                    live = slot_msg >= 0
                    if pipelined:
                        if pending is not None:
                            ev, msg_then, fed_then = pending
                            ev.synchronize()
                            done = live & (slot_msg == msg_then) & (fed_then >= nlen_host)
                        else:
                            ev, done = None, np.zeros(slot_msg.shape, dtype=bool)
                    else:
                        ev, done = None, live & ((lm.kv.lens_host - ctx_host) >= nlen_host)
                    fin = np.nonzero(done)[0]
                    if fin.size:
                        if ev is not None:
                            srows = _rows_after(ev, side, st["state"], fin).numpy()
                            f = _state_fields(torch.from_numpy(srows))
                            rows = _rows_after(ev, side, st["out_bits"], fin)
                        else:
                            f = _state_fields(st["state"][torch.as_tensor(fin, device=dev)])
                            rows = st["out_bits"][torch.as_tensor(fin, device=dev)]
                        bad = fin[(f["flags"] & L.NS_ST_ERR_DIVERGE) != 0]
                        if bad.size:
                            raise DecodeDivergenceError(
                                f"streams {slot_msg[bad].tolist()[:8]}: received token outside the kept top-k")
                        got = _bit_rows_to_lists(rows, f["bit_pos"])
                        for j, s in enumerate(fin.tolist()):
                            out[int(slot_msg[s])] = got[j]
                        lm.kv.release(fin)
                        slot_msg[fin] = -1
                        nlen_host[fin] = 0
                        admit_blocked = False
                        fi = torch.as_tensor(fin, device=dev)
                        st["nlen"][fi] = 0
                        st["stop"][fi] = 0
                        live = slot_msg >= 0
                    empty = np.nonzero(~live)[0]
                    if queue and empty.size and not admit_blocked:
                        room = lm.pool.free_pages + lm.pool.growable_pages() - int(live.sum()) - 1
                        if per_ctx:
                            adm_m = _admissible(queue, self.contexts, self.ahead - 1, empty.size, room,
                                                self.keys, self.shares, lm.kv.entries, self.chains,
                                                lm.kv.prefixes)
                            if adm_m:
                                back = self._admit_contexts(st, carry, init_row, empty[:len(adm_m)], adm_m, slot_msg,
                                                            nlen_host, ctx_host, Tcap)
                                queue.extendleft(reversed(back))
                                admit_blocked = bool(back)
                                live = slot_msg >= 0
                            if not live.any():
                                m = queue[0]
                                raise KVCapacityError(
                                    f"message {m}: no device memory for the KV pages of its "
                                    f"{len(self.contexts[m])}-token context")
                        else:
                            n_adm = int(min(empty.size, len(queue), max(0, room)))
                            if n_adm:
                                adm_s = empty[:n_adm]
                                adm_m = [queue.popleft() for _ in range(n_adm)]
                                lm.kv.reset(adm_s)
                                self._admit(st, carry, first, init_row, adm_s, adm_m, slot_msg, nlen_host, T0, Tcap)
                                live = slot_msg >= 0
                    # pages for the next (check_every + 1) * C positions, never past a message's last token
                    while live.any():
                        sl = np.nonzero(live)[0]
                        upto = chunk_page_horizon(lm.kv.lens_host[sl], ctx_host[sl] + nlen_host[sl],
                                                  self.check_every, C)
                        if lm.kv.ensure(sl, upto).size == 0:
                            break
                        if sl.size == 1:
                            raise KVCapacityError(f"message {int(slot_msg[sl[0]])} ({int(nlen_host[sl[0]])} tokens) "
                                                  "needs more KV pages than the device holds")
                        v = sl[np.argmin(lm.kv.lens_host[sl] - ctx_host[sl])]  # the youngest: fewest tokens fed
                        queue.appendleft(int(slot_msg[v]))
                        lm.kv.release([v])
                        vi = torch.as_tensor([int(v)], device=dev)
                        st["nlen"][vi] = 0
                        st["stop"][vi] = 0
                        slot_msg[v], nlen_host[v] = -1, 0
                        live = slot_msg >= 0
                        admit_blocked = True
                        self.evictions += 1
                    if not live.any():
                        break
                    if self.allow_compact and not queue and int(live.sum()) <= st["state"].shape[0] // 2 and \
                            st["state"].shape[0] > 1:
                        keep = np.nonzero(live)[0]
                        lm.kv.release(np.setdiff1d(np.arange(st["state"].shape[0]), keep))
                        lm.kv.compact(keep)
                        lm.B = lm.kv.B
                        ki = torch.as_tensor(keep, device=dev)
                        for k in st:
                            st[k] = st[k].index_select(0, ki).contiguous()
                        carry = carry.index_select(0, ki).contiguous()
                        logits = torch.zeros((keep.size, C, lm.ld), device=dev, dtype=lm.logits_dtype)
                        slot_msg, nlen_host = slot_msg[keep].copy(), nlen_host[keep].copy()
                        ctx_host = ctx_host[keep].copy()
                        self.compactions += 1
                    if pipelined:
                        ev_now = torch.cuda.Event()
                        ev_now.record()
                        pending = (ev_now, slot_msg.copy(), lm.kv.lens_host - ctx_host)
                key = _layout_key(carry, logits, st["state"], st["tokmat"], lm.kv.table, lm.kv.lens, st.get("ctx"),
                                  st.get("quality")) + (lm.kv.version,)
                if self.use_graph:
                    if graph is None or key != gkey:
                        graph = None
                        lm.begin_chunk_static(logits)
                        graph, gkey = _SlotGraph(body), key
                    else:
                        graph.replay()
                else:
                    lm.begin_chunk_static(logits)
                    body()
                # the host mirror of ``lens += cnt``: a slot of an evicted or finished message has nlen 0 and stays
                lm.advance_rows(chunk_counts(lm.kv.lens_host - ctx_host, nlen_host, C))
                t += 1
        finally:
            if graph is not None:
                torch.cuda.current_stream().synchronize()
            del graph
        return out

    def _admit_contexts(self, st, logits, init_row, slots, msgs, slot_msg, nlen_host, ctx_host, Tcap):
        """Admit ``msgs`` with their own contexts into ``slots``: pages for each context and the message's first
        positions, one ragged prefill into those pages, then the slot state of :meth:`_admit` with a per-slot context
        length.  Returns the messages that could not be given pages."""
        import torch

        lm = self.lm
        slots = np.asarray(slots, dtype=np.int64)
        tl = np.asarray([len(self.contexts[m]) for m in msgs], dtype=np.int64)
        nl = np.asarray([len(self.lists[m]) for m in msgs], dtype=np.int64)
        chains = [self.chains[m] for m in msgs] if self.chains is not None else None
        ok = _map_contexts(lm.kv, slots, [self.keys[m] for m in msgs], [self.shares[m] for m in msgs], tl,
                           tl + np.minimum(self.ahead, nl), chains)
        back = [m for m, k in zip(msgs, ok) if not k]
        slots, msgs, tl = slots[ok], [m for m, k in zip(msgs, ok) if k], tl[ok]
        if not msgs:
            return back
        first = lm.prefill_contexts([self.contexts[m] for m in msgs], slots, [self.shares[m] for m in msgs],
                                    [self.chains[m] for m in msgs] if self.chains is not None else None)
        self.prefix_rows_saved += lm.last_prefill.get("prefix_rows_saved", 0)
        self.prefix_entries += lm.last_prefill.get("prefix_entries", 0)
        self.prefill_rows += lm.last_prefill["rows"]
        self.prefill_groups += lm.last_prefill["groups"]
        self.prefill_shared += lm.last_prefill["shared"]
        idx = torch.as_tensor(slots, device=logits.device)
        st["ctx"][idx] = torch.from_numpy(tl.astype(np.int32)).to(logits.device)
        ctx_host[slots] = tl
        self._admit(st, logits, first, init_row, slots, msgs, slot_msg, nlen_host, tl, Tcap)
        return back

    def _admit(self, st, logits, first, init_row, slots, msgs, slot_msg, nlen_host, T0, Tcap):
        """``T0``: the context length of the admitted messages (the shared one, or one per slot); ``first``: the
        context's ``[1, ld]`` logits, or one row per slot."""
        import torch

        dev = logits.device
        n = len(slots)
        mat = np.zeros((n, Tcap), dtype=np.int32)
        nl = np.zeros(n, dtype=np.int64)
        for i, m in enumerate(msgs):
            tl = self.lists[m]
            nl[i] = len(tl)
            if len(tl):
                mat[i, : len(tl)] = np.asarray(tl, dtype=np.int32)
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        st["tokmat"][idx] = torch.from_numpy(mat).to(dev)
        nlt = torch.from_numpy(nl.astype(np.int32)).to(dev)
        st["nlen"][idx] = nlt
        t0 = T0 if np.isscalar(T0) else torch.from_numpy(np.asarray(T0).astype(np.int32)).to(dev)
        st["stop"][idx] = nlt + (t0 - 1)
        if self.qual is not None:  # the messages' quality rows, and fresh states at each row's 2^precision
            rows = self.qual.take(list(msgs))
            st["quality"][idx] = rows.table(dev)
            st["state"][idx] = rows.init_rows(dev)
        else:
            st["state"][idx] = init_row.expand(n, 4)
        st["out_bits"][idx] = 0
        logits.index_copy_(0, idx, first.expand(n, -1).to(logits.dtype))
        slot_msg[slots] = msgs
        nlen_host[slots] = nl


class SlotSampler:
    """Sample ``lengths[m]`` tokens after ``contexts[m]`` for every message through ``slots`` slots, longest first.
    Closest to :class:`SlotDecoder`: a message's end is known on the host from its length, so the loop never reads
    the coder states -- a slot counts as finished once the event recorded at the previous check has passed with its
    last token drawn.  On the device a stream past its length is PARKED by the step itself
    (``ns_sample_step_streams``: nothing of it is written) and its attention is skipped through the per-stream stop
    position, which is what lets ``check_every`` steps run without a host check.

    Every message has its own context (a shared one is the same context N times: its pages are then shared), its
    own row of the quality table (temperature, top-k) and of the draw table (seed, draw id, length).  Draws are keyed
    by (seed, draw id, token index) and by nothing else, so a message gives the same tokens in any slot, and an
    evicted message -- re-queued, restarted from token 0 -- gives them again."""

    def __init__(self, provider, ctx, contexts: Sequence[Sequence[int]], lengths: Sequence[int], qualities, seeds,
                 gids, *, slots: int, use_graph: bool, stats: bool, check_every: int = 16, compact: bool = True,
                 share: bool = True, share_prefixes: bool = True):
        self.p, self.lm, self.ctx = provider, provider.lm, ctx
        self.qual = qualities  # coder.StreamQuality, one row per message
        self.N = len(lengths)
        self.S = max(1, min(int(slots), self.N))
        self.lengths = np.asarray([int(v) for v in lengths], dtype=np.int64)
        self.seeds, self.gids = [int(s) for s in seeds], [int(g) for g in gids]
        self.contexts = _trimmed(contexts, self.N)
        self.keys, self.shares = _multiplicity(self.contexts, share)
        self.chains = _prefix_chains(self.contexts, share and share_prefixes and
                                     getattr(self.lm, "prefix_sharing", False))
        self.prefix_rows_saved = self.prefix_entries = 0
        self.prefill_shared = self.prefill_rows = self.prefill_groups = 0
        self.use_graph, self.stats = use_graph, stats
        self.check_every, self.allow_compact = int(check_every), compact
        self.compactions = self.evictions = self.kv_peak = 0

    def run(self):
        import torch

        lm, S, N = self.lm, self.S, self.N
        Lmax = int(self.lengths.max())
        order = np.argsort(-self.lengths, kind="stable")  # longest first: the tail is short messages
        # initial token-history / page-table width (both grow on demand; a provider may set a small one in tests)
        budget = getattr(self.p, "slot_budget_tokens", None) or Lmax + 1
        lm.begin_slots(S, 0, budget)
        logits = torch.zeros((S, lm.ld), device=lm.device, dtype=lm.logits_dtype)
        dev = logits.device
        # every slot starts parked (length 0) on a valid quality row
        sess = self._session(S, int(budget), Lmax)
        stop = torch.zeros(S, dtype=torch.int32, device=dev)
        ctx_host = np.zeros(S, dtype=np.int64)
        len_host = np.zeros(S, dtype=np.int64)
        slot_msg = np.full(S, -1, dtype=np.int64)
        queue = deque(order.tolist())
        tokens: List[Optional[List[int]]] = [None] * N
        stats_out: List[Optional[dict]] = [None] * N
        graph, gkey = None, None
        admit_blocked = False

        def body():
            lm.step_static(sess.step(logits))

        def park(sl):
            sess.park_slots(sl)
            stop[torch.as_tensor(np.asarray(sl, dtype=np.int64), device=dev)] = 0
            len_host[sl] = 0

        t = 0
        pipelined = self.use_graph
        side = torch.cuda.Stream() if pipelined else None
        pending = None
        try:
            while True:
                if t % self.check_every == 0:
                    live = slot_msg >= 0
                    if pipelined:
                        if pending is not None:
                            ev, msg_then, fed_then = pending
                            ev.synchronize()
                            done = live & (slot_msg == msg_then) & (fed_then >= len_host)
                        else:
                            ev, done = None, np.zeros(slot_msg.shape, dtype=bool)
                    else:
                        ev, done = None, live & ((lm.kv.lens_host - ctx_host) >= len_host)
                    fin = np.nonzero(done)[0]
                    if fin.size:
                        nl = len_host[fin]
                        got, acc = self._harvest(sess, fin, nl, ev, side, slot_msg[fin])
                        for j, s in enumerate(fin.tolist()):
                            m = int(slot_msg[s])
                            tokens[m] = got[j]
                            if self.stats:
                                stats_out[m] = _stats_rows(acc[j:j + 1])[0]
                        lm.kv.release(fin)
                        slot_msg[fin] = -1
                        park(fin)
                        admit_blocked = False
                        live = slot_msg >= 0
                    empty = np.nonzero(~live)[0]
                    if queue and empty.size and not admit_blocked:
                        room = lm.pool.free_pages + lm.pool.growable_pages() - int(live.sum()) - 1
                        adm = _admissible(queue, self.contexts, self.check_every, empty.size, room, self.keys,
                                          self.shares, lm.kv.entries, self.chains, lm.kv.prefixes)
                        if adm:
                            back = self._admit_contexts(sess, logits, stop, empty[:len(adm)], adm, slot_msg, len_host,
                                                        ctx_host)
                            queue.extendleft(reversed(back))
                            admit_blocked = bool(back)
                            live = slot_msg >= 0
                        if not live.any():
                            m = queue[0]
                            raise KVCapacityError(
                                f"message {m}: no device memory for the KV pages of its "
                                f"{len(self.contexts[m])}-token context")
                    # pages for the next check_every + 1 positions (never past a message's last drawn token); on a
                    # full device the youngest messages go back to the queue's front (sampled again from token 0:
                    # the same tokens, their draws are keyed by seed, draw id and token index)
                    while live.any():
                        sl = np.nonzero(live)[0]
                        upto = np.minimum(lm.kv.lens_host[sl] + self.check_every + 1, ctx_host[sl] + len_host[sl])
                        if lm.kv.ensure(sl, upto).size == 0:
                            break
                        if sl.size == 1:
                            raise KVCapacityError(f"message {int(slot_msg[sl[0]])} ({int(len_host[sl[0]])} tokens) "
                                                  "needs more KV pages than the device holds")
                        v = sl[np.argmin(lm.kv.lens_host[sl] - ctx_host[sl])]  # the youngest: fewest tokens drawn
                        queue.appendleft(int(slot_msg[v]))
                        lm.kv.release([v])
                        park(np.asarray([v]))
                        slot_msg[v] = -1
                        live = slot_msg >= 0
                        admit_blocked = True
                        self.evictions += 1
                    if not live.any():
                        break
                    if self.allow_compact and not queue and int(live.sum()) <= sess.B // 2 and sess.B > 1:
                        keep = np.nonzero(live)[0]
                        lm.kv.release(np.setdiff1d(np.arange(sess.B), keep))
                        lm.kv.compact(keep)
                        lm.B = lm.kv.B
                        sess.compact(keep)
                        ki = torch.as_tensor(keep, device=dev)
                        stop = stop.index_select(0, ki).contiguous()
                        logits = logits.index_select(0, ki).contiguous()
                        slot_msg, len_host = slot_msg[keep].copy(), len_host[keep].copy()
                        ctx_host = ctx_host[keep].copy()
                        self.compactions += 1
                    lm.stop_len = stop  # a parked slot skips its attention (and appends no K/V)
                    if pipelined:
                        ev_now = torch.cuda.Event()
                        ev_now.record()
                        pending = (ev_now, slot_msg.copy(), lm.kv.lens_host - ctx_host)
                key = self._key(sess) + _layout_key(logits, stop, lm.kv.table, lm.kv.lens) + (lm.kv.version,)
                if self.use_graph:
                    if graph is None or key != gkey:
                        graph = None
                        lm.begin_static(logits)
                        graph, gkey = _SlotGraph(body), key
                    else:
                        graph.replay()
                else:
                    lm.begin_static(logits)
                    body()
                lm.advance(1)
                t += 1
        finally:
            if graph is not None:
                torch.cuda.current_stream().synchronize()
            lm.stop_len = None
            del graph
        self.kv_peak = lm.kv.peak
        return tokens, (stats_out if self.stats else None)

    # what a subclass with another coder session replaces (RankSlotDecoder)
    def _session(self, S: int, budget: int, Lmax: int):
        """The coder session of the run: every slot parked (length 0) on a valid quality row."""
        from ..coder import SampleSession

        return SampleSession(self.ctx, S, max_tokens=max(1, min(int(budget), Lmax)), stats=self.stats,
                             quality=self.qual.take([0] * S), seeds=[0] * S, gids=[0] * S, lengths=[0] * S)

    def _harvest(self, sess, fin, nl, ev, side, msgs):
        """``(results, accumulators or None)`` of the finished slots ``fin`` (messages ``msgs``, lengths ``nl``); with
        ``ev`` (the pipelined check) gathered on the ``side`` stream once the event has passed."""
        if ev is not None:
            host = _rows_after(ev, side, sess.hist, fin, int(nl.max())).numpy()
            acc = _rows_after(ev, side, sess.stats_acc, fin).numpy() if self.stats else None
            return [host[j, : int(nl[j])].tolist() for j in range(fin.size)], acc
        return sess.harvest(fin, nl)

    def _key(self, sess) -> tuple:
        return _layout_key(sess.state, sess.hist, sess.out_token, sess.stats_acc, sess.qtable, sess.draws)

    def _load(self, sess, slots, msgs, nl) -> None:
        sess.load_slots(slots, self.qual.take(msgs), [self.seeds[m] for m in msgs], [self.gids[m] for m in msgs], nl)

    def _admit_contexts(self, sess, logits, stop, slots, msgs, slot_msg, len_host, ctx_host):
        """Admit ``msgs`` into ``slots``: pages for each context and the message's first positions, one ragged prefill
        of the contexts into those pages, the messages' quality and draw rows with fresh states, each context's
        logits into its slot's row.  Returns the messages that could not be given pages (back to the queue)."""
        import torch

        lm = self.lm
        slots = np.asarray(slots, dtype=np.int64)
        tl = np.asarray([len(self.contexts[m]) for m in msgs], dtype=np.int64)
        nl = self.lengths[np.asarray(msgs, dtype=np.int64)]
        chains = [self.chains[m] for m in msgs] if self.chains is not None else None
        ok = _map_contexts(lm.kv, slots, [self.keys[m] for m in msgs], [self.shares[m] for m in msgs], tl,
                           tl + np.minimum(self.check_every + 1, nl), chains)
        back = [m for m, k in zip(msgs, ok) if not k]
        slots, msgs, tl, nl = slots[ok], [m for m, k in zip(msgs, ok) if k], tl[ok], nl[ok]
        if not msgs:
            return back
        first = lm.prefill_contexts([self.contexts[m] for m in msgs], slots, [self.shares[m] for m in msgs],
                                    [self.chains[m] for m in msgs] if self.chains is not None else None)
        self.prefix_rows_saved += lm.last_prefill.get("prefix_rows_saved", 0)
        self.prefix_entries += lm.last_prefill.get("prefix_entries", 0)
        self.prefill_rows += lm.last_prefill["rows"]
        self.prefill_groups += lm.last_prefill["groups"]
        self.prefill_shared += lm.last_prefill["shared"]
        self._load(sess, slots, msgs, nl)
        idx = torch.as_tensor(slots, device=logits.device)
        # the attention is skipped once the cache length reaches context + length - 1: the logits after the last
        # drawn token are never read
        stop[idx] = torch.from_numpy((tl + nl - 1).astype(np.int32)).to(logits.device)
        logits.index_copy_(0, idx, first.to(logits.dtype))
        slot_msg[slots] = msgs
        ctx_host[slots] = tl
        len_host[slots] = nl
        return back


class RankSlotEncoder(SlotEncoder):
    """:class:`SlotEncoder` over the rank coder (``coder.RankStreamEncodeSession``, ``ns_rank_encode_step_streams``):
    every message has its own context and its own row of the rank quality table (temperature and policy).  The loop --
    admission, shared pages, the pipelined check, graph capture, eviction, compaction -- is the parent's; a finished
    slot hands over its consumption history (the reference's ``state["history"]``) with its tokens.  The step depends
    on nothing but the stream's own logits, payload and row, so a message gives the tokens of its one-message call in
    any slot, and an evicted message gives them again."""

    def __init__(self, provider, ctx, bit_lists, contexts, qualities, *, slots: int, use_graph: bool,
                 check_every: int = 16, compact: bool = True, share: bool = True, share_prefixes: bool = True):
        max_bits = max(len(b) for b in bit_lists)
        # a rank stream consumes at least one bit per token: it never stalls and never exceeds its bit count
        super().__init__(provider, ctx, bit_lists, None, slots=slots, finish=False, stop_text=None, stats=False,
                         check_every=check_every, stall_steps=1 << 30, hard_cap=max_bits + 64, use_graph=use_graph,
                         compact=compact, contexts=contexts, share=share, qualities=qualities,
                         share_prefixes=share_prefixes)
        self.consumed: List[Optional[List[int]]] = [None] * self.N

    def _session(self, S: int, budget: int, stride: int):
        from ..coder import RankStreamEncodeSession

        return RankStreamEncodeSession(self.ctx, S, payload_stride=stride, max_tokens=budget)

    def _range_error(self, msgs) -> str:
        return f"messages {msgs}: language model distribution provides no capacity"

    def _harvested(self, sess, fin, msgs, nt, ev, side) -> None:
        import torch

        ncol = max(1, int(nt.max()))
        if ev is not None:
            host = _rows_after(ev, side, sess.cons, fin, ncol).numpy()
        else:
            host = sess.cons[torch.as_tensor(fin, device=sess.cons.device), :ncol].cpu().numpy()
        for j, m in enumerate(msgs.tolist()):
            self.consumed[int(m)] = host[j, : int(nt[j])].tolist()

    def _key_extra(self, sess) -> tuple:
        return _layout_key(sess.cons, sess.nbits, sess.out_token)


class RankSlotDecoder(SlotSampler):
    """:class:`SlotSampler`'s loop over the rank decoder (``coder.RankStreamDecodeSession``,
    ``ns_rank_decode_step_streams``): a message's end is known on the host from its token count, a slot past its last
    token is inactive on the device, and every message has its own context, consumption history and row of the rank
    quality table.  ``run()`` returns each message's decoded bytes."""

    def __init__(self, provider, ctx, token_lists, histories, contexts, qualities, *, slots: int, use_graph: bool,
                 check_every: int = 16, compact: bool = True, share: bool = True, share_prefixes: bool = True):
        n = len(token_lists)
        super().__init__(provider, ctx, contexts, [len(t) for t in token_lists], qualities, [0] * n, [0] * n,
                         slots=slots, use_graph=use_graph, stats=False, check_every=check_every, compact=compact,
                         share=share, share_prefixes=share_prefixes)
        self.lists = token_lists
        self.hists = [list(h)[: len(t)] for t, h in zip(token_lists, histories)]

    def _session(self, S: int, budget: int, Lmax: int):
        from ..coder import RankStreamDecodeSession

        return RankStreamDecodeSession(self.ctx, S, max_tokens=Lmax,
                                       max_bits=max((sum(h) for h in self.hists), default=0))

    def _harvest(self, sess, fin, nl, ev, side, msgs):
        from ..codec.errors import DecodeDivergenceError
        from ..coder import RankStreamDecodeSession

        if ev is not None:
            st, ob = _rows_after(ev, side, sess.state, fin), _rows_after(ev, side, sess.out_bits, fin)
            flags = _state_fields(st)["flags"]
            got = RankStreamDecodeSession.payloads_of(st, ob)
        else:
            got, flags = sess.harvest(fin)
        bad = msgs[(flags & _lib.NS_ST_ERR_DIVERGE) != 0]
        if bad.size:
            raise DecodeDivergenceError(f"messages {bad.tolist()[:8]}: token not present in distribution")
        return got, None

    def _key(self, sess) -> tuple:
        return _layout_key(sess.state, sess.tokmat, sess.keepmat, sess.nlen, sess.out_bits, sess.qtable)

    def _load(self, sess, slots, msgs, nl) -> None:
        sess.load_slots(slots, [self.lists[m] for m in msgs], [self.hists[m] for m in msgs], self.qual.take(msgs))


class SlotRevealer:
    """Find the spans of many cover texts through ``slots`` slots (``coder.DecodeStreamsSession``,
    ``ns_decode_step_streams``).  A unit of work is (text i, its remaining ids): one slot decodes it after text i's
    context with text i's quality row.  Unlike the other decode loops the end of a unit is not known in advance -- a
    span ends where the decoded packet's JSON closes (plus the ``finish_sent`` tail) -- so every host check gathers,
    for every live slot, the state, the bits up to ``bit_pos`` and the bit count after each decoded token (written by
    the coder kernel itself), and asks ``cover._span_end``:

    * the span settles at ``end``: ``ids[:end + 1]`` is recorded, the slot's pages are released and
      ``ids[end + 1:]`` is queued as a fresh stream of the same text -- the same context (prefilled again, or shared
      through the registry with whoever holds it), a reset coder state.  The tokens decoded past ``end`` before the
      check (the next span's, out of context) are discarded, as the round-based path discards them;
    * the slot is flagged ``NS_ST_ERR_DIVERGE`` (or ``NS_ST_ERR_RANGE``) and nothing settled from the counts before
      it: the text leaves the batch and its current remainder goes, unchanged, to ``fallback`` (the caller runs the
      round-based code with the BPE repair on it).  A flag at or after a settled ``end`` is ignored;
    * the remainder is fully decoded and nothing settled: ``DecodeDivergenceError`` ("no complete packet ...").

    The loop -- admission, shared pages, the pipelined check, graph capture, eviction of the youngest on a full
    device, compaction once the queue is drained -- is :class:`SlotSampler`'s.  The check reads a copy of the three
    buffers taken in stream order at the PREVIOUS check (consistent among themselves), so a span is noticed one check
    late and the GPU never waits for the host.  An evicted text is re-queued with its current remainder and decoded
    again from that remainder's start: the same bits, a stream's result does not depend on its neighbours."""

    def __init__(self, provider, ctx, id_lists, contexts, qualities, finishes, sent_end, *, slots: int,
                 use_graph: bool, labels=None, check_every: int = 16, compact: bool = True, share: bool = True,
                 share_prefixes: bool = True):
        self.p, self.lm, self.ctx = provider, provider.lm, ctx
        self.qual = qualities  # coder.StreamQuality, one row per text
        self.N = len(id_lists)
        self.S = max(1, min(int(slots), self.N))
        self.rest = [[int(t) for t in ids] for ids in id_lists]
        self.finish = [bool(f) for f in finishes]
        self.sent_end = sent_end
        self.labels = list(labels) if labels is not None else list(range(self.N))
        self.contexts = _trimmed(contexts, self.N)
        self.keys, self.shares = _multiplicity(self.contexts, share)
        self.chains = _prefix_chains(self.contexts, share and share_prefixes and
                                     getattr(self.lm, "prefix_sharing", False))
        self.use_graph = use_graph
        self.check_every, self.allow_compact = int(check_every), compact
        self.spans: List[List[List[int]]] = [[] for _ in range(self.N)]
        self.fallback: List[int] = []  # texts that left the batch on a divergence (their remainder is in ``rest``)
        self.steps = self.discarded = self.prefill_rows = 0
        self.compactions = self.evictions = self.kv_peak = 0

    def run(self) -> List[List[List[int]]]:
        import torch

        from ..codec.errors import DecodeDivergenceError
        from ..coder import DecodeStreamsSession
        from ..cover import _span_end
        from ..exceptions import PacketECCError
        from ..stego import packet_prefix

        lm, S = self.lm, self.S
        Lmax = max(1, max(len(r) for r in self.rest))
        order = np.argsort(-np.asarray([len(r) for r in self.rest]), kind="stable")  # longest first
        budget = getattr(self.p, "slot_budget_tokens", None) or Lmax + 1
        lm.begin_slots(S, 0, budget)
        logits = torch.zeros((S, lm.ld), device=lm.device, dtype=lm.logits_dtype)
        dev = logits.device
        sess = DecodeStreamsSession(self.ctx, S, max_tokens=Lmax, k_max=self.qual.k_max,
                                    max_precision=self.qual.max_precision, rank_export=False)
        stop = torch.zeros(S, dtype=torch.int32, device=dev)
        ctx_host = np.zeros(S, dtype=np.int64)
        len_host = np.zeros(S, dtype=np.int64)
        slot_msg = np.full(S, -1, dtype=np.int64)
        slot_gen = np.zeros(S, dtype=np.int64)  # admissions per slot: a copy belongs to the unit it was taken of
        queue = deque(i for i in order.tolist() if self.rest[i])
        graph, gkey = None, None
        admit_blocked = False
        bad = _lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_ERR_RANGE
        pins = (_Pinned(), _Pinned(), _Pinned())

        def body():
            lm.step_static(sess.step(logits))

        def park(sl):
            sess.park_slots(sl)
            stop[torch.as_tensor(np.asarray(sl, dtype=np.int64), device=dev)] = 0
            len_host[sl] = 0

        def copy_out():
            """The three buffers as they stand in stream order now, on their way to pinned host memory."""
            got = [pin.take(t) for pin, t in zip(pins, (sess.state, sess.out_bits, sess.counts))]
            return got[-1][1], [g[0] for g in got], slot_gen.copy()

        def packet_closed(data: bytes) -> bool:
            """Whether the whole bytes decoded so far (LSB-first bits: the buffer's own bytes) begin with a complete
            packet -- ``_span_end``'s own first test, on the same bytes."""
            try:
                packet_prefix(data)
            except PacketECCError:
                return False
            return True

        def settle(snap):
            """Ask ``_span_end`` for every live slot whose unit the copy was taken of; returns the freed slots."""
            ev, (st_h, ob_h, cn_h), gen_then = snap
            ev.synchronize()
            f = _state_fields(st_h)
            ob, cn = ob_h.numpy(), cn_h.numpy()
            freed = []
            for s in np.nonzero((slot_msg >= 0) & (slot_gen == gen_then))[0].tolist():
                i = int(slot_msg[s])
                ids = self.rest[i]
                nt = min(int(f["ntokens"][s]), len(ids))
                flagged = bool(int(f["flags"][s]) & bad)
                if nt == 0 and not flagged:
                    continue
                bp = int(f["bit_pos"][s])
                end = None
                if packet_closed(ob[s, : bp // 8].tobytes()):  # else _span_end has nothing to find: skip its bit loop
                    bits = np.unpackbits(ob[s, : (bp + 7) // 8], bitorder="little")[:bp].tolist()
                    end = _span_end(bits, cn[s, :nt].tolist(), ids, self.finish[i], self.sent_end)
                if end is not None:
                    self.spans[i].append(ids[: end + 1])
                    self.rest[i] = ids[end + 1:]
                    fed = int(lm.kv.lens_host[s] - ctx_host[s]) if not flagged else nt
                    self.discarded += max(0, min(fed, len(ids)) - (end + 1))
                    if self.rest[i]:
                        queue.append(i)
                elif flagged:
                    self.fallback.append(i)
                elif nt >= len(ids):
                    raise DecodeDivergenceError(
                        f"cover {self.labels[i]}: no complete packet in the remaining {len(ids)} tokens")
                else:
                    continue
                freed.append(s)
            return np.asarray(freed, dtype=np.int64)

        t = 0
        pipelined = self.use_graph
        pending = None
        try:
            while True:
                if t % self.check_every == 0:
                    snap = pending if pipelined else (copy_out() if t else None)
                    fin = settle(snap) if snap is not None else np.zeros(0, dtype=np.int64)
                    if fin.size:
                        lm.kv.release(fin)
                        slot_msg[fin] = -1
                        park(fin)
                        admit_blocked = False
                    live = slot_msg >= 0
                    empty = np.nonzero(~live)[0]
                    if queue and empty.size and not admit_blocked:
                        room = lm.pool.free_pages + lm.pool.growable_pages() - int(live.sum()) - 1
                        adm = _admissible(queue, self.contexts, self.check_every, empty.size, room, self.keys,
                                          self.shares, lm.kv.entries, self.chains, lm.kv.prefixes)
                        if adm:
                            back = self._admit(sess, logits, stop, empty[:len(adm)], adm, slot_msg, slot_gen, len_host,
                                               ctx_host)
                            queue.extendleft(reversed(back))
                            admit_blocked = bool(back)
                            live = slot_msg >= 0
                        if not live.any():
                            m = queue[0]
                            raise KVCapacityError(
                                f"cover {self.labels[m]}: no device memory for the KV pages of its "
                                f"{len(self.contexts[m])}-token context")
                    # pages for the next check_every + 1 positions (never past a unit's last token); on a full device
                    # the youngest units go back to the queue's front (decoded again from their remainder's start)
                    while live.any():
                        sl = np.nonzero(live)[0]
                        upto = np.minimum(lm.kv.lens_host[sl] + self.check_every + 1, ctx_host[sl] + len_host[sl])
                        if lm.kv.ensure(sl, upto).size == 0:
                            break
                        if sl.size == 1:
                            raise KVCapacityError(f"cover {self.labels[int(slot_msg[sl[0]])]} "
                                                  f"({int(len_host[sl[0]])} tokens left) needs more KV pages than the "
                                                  "device holds")
                        v = sl[np.argmin(lm.kv.lens_host[sl] - ctx_host[sl])]  # the youngest: fewest tokens decoded
                        queue.appendleft(int(slot_msg[v]))
                        lm.kv.release([v])
                        park(np.asarray([v]))
                        slot_msg[v] = -1
                        live = slot_msg >= 0
                        admit_blocked = True
                        self.evictions += 1
                    if not live.any():
                        break
                    if self.allow_compact and not queue and int(live.sum()) <= sess.B // 2 and sess.B > 1:
                        keep = np.nonzero(live)[0]
                        lm.kv.release(np.setdiff1d(np.arange(sess.B), keep))
                        lm.kv.compact(keep)
                        lm.B = lm.kv.B
                        sess.compact(keep)
                        ki = torch.as_tensor(keep, device=dev)
                        stop = stop.index_select(0, ki).contiguous()
                        logits = logits.index_select(0, ki).contiguous()
                        slot_msg, len_host = slot_msg[keep].copy(), len_host[keep].copy()
                        ctx_host, slot_gen = ctx_host[keep].copy(), slot_gen[keep].copy()
                        self.compactions += 1
                    lm.stop_len = stop  # a parked slot skips its attention (and appends no K/V)
                    if pipelined:
                        pending = copy_out()
                key = _layout_key(sess.state, sess.tokmat, sess.nlen, sess.counts, sess.out_bits, sess.out_token,
                                  sess.qtable, logits, stop, lm.kv.table, lm.kv.lens) + (lm.kv.version,)
                if self.use_graph:
                    if graph is None or key != gkey:
                        graph = None
                        lm.begin_static(logits)
                        graph, gkey = _SlotGraph(body), key
                    else:
                        graph.replay()
                else:
                    lm.begin_static(logits)
                    body()
                lm.advance(1)
                t += 1
        finally:
            if graph is not None:
                torch.cuda.current_stream().synchronize()
            lm.stop_len = None
            del graph
        self.steps = t
        self.kv_peak = lm.kv.peak
        return self.spans

    def _admit(self, sess, logits, stop, slots, msgs, slot_msg, slot_gen, len_host, ctx_host):
        """Admit the texts ``msgs`` (their current remainders) into ``slots``: pages for each context and the unit's
        first positions, one ragged prefill of the contexts into those pages, each text's quality row and tokens with
        a fresh coder state, each context's logits into its slot's row.  Returns the texts that could not be given
        pages (back to the queue)."""
        import torch

        lm = self.lm
        slots = np.asarray(slots, dtype=np.int64)
        tl = np.asarray([len(self.contexts[m]) for m in msgs], dtype=np.int64)
        nl = np.asarray([len(self.rest[m]) for m in msgs], dtype=np.int64)
        chains = [self.chains[m] for m in msgs] if self.chains is not None else None
        ok = _map_contexts(lm.kv, slots, [self.keys[m] for m in msgs], [self.shares[m] for m in msgs], tl,
                           tl + np.minimum(self.check_every + 1, nl), chains)
        back = [m for m, k in zip(msgs, ok) if not k]
        slots, msgs, tl, nl = slots[ok], [m for m, k in zip(msgs, ok) if k], tl[ok], nl[ok]
        if not msgs:
            return back
        first = lm.prefill_contexts([self.contexts[m] for m in msgs], slots, [self.shares[m] for m in msgs],
                                    [self.chains[m] for m in msgs] if self.chains is not None else None)
        self.prefill_rows += lm.last_prefill["rows"]
        sess.load_slots(slots, [self.rest[m] for m in msgs], self.qual.take(msgs))
        idx = torch.as_tensor(slots, device=logits.device)
        # the attention is skipped once the cache length reaches context + tokens - 1: the logits after the unit's
        # last token are never read
        stop[idx] = torch.from_numpy((tl + nl - 1).astype(np.int32)).to(logits.device)
        logits.index_copy_(0, idx, first.to(logits.dtype))
        slot_msg[slots] = msgs
        slot_gen[slots] += 1
        ctx_host[slots] = tl
        len_host[slots] = nl
        return back


class BaselineSlotEncoder(SlotEncoder):
    """:class:`SlotEncoder` over a fixed-block baseline coder (``coder.BaselineEncodeSession``: the Huffman coder of
    ``code_base/huffman_baseline.py`` or the bins coder of ``code_base/block_baseline.py``).  The loop -- admission,
    one context per message, shared context pages and prefixes, the pipelined check, graph capture, eviction,
    compaction -- is the parent's.  The step depends on nothing but the stream's own logits and payload, so a message
    gives the tokens, bits and statistics of its one-message call in any slot, and an evicted message gives them
    again."""

    def __init__(self, provider, ctx, bit_lists, context, *, mode: str, block_size: int, slots: int, finish: bool,
                 stats: bool, use_graph: bool, check_every: int = 16, compact: bool = True, contexts=None,
                 share: bool = True, share_prefixes: bool = True, stall_steps: int = 4096):
        max_bits = max(len(b) for b in bit_lists)
        # a baseline stream consumes at least one bit per token; only a finish_sent tail can run on
        super().__init__(provider, ctx, bit_lists, context, slots=slots, finish=finish, stop_text=None, stats=stats,
                         check_every=check_every, stall_steps=stall_steps, hard_cap=max_bits + stall_steps + 64,
                         use_graph=use_graph, compact=compact, contexts=contexts, share=share, qualities=None,
                         share_prefixes=share_prefixes)
        self.mode, self.block_size = mode, int(block_size)

    def _session(self, S: int, budget: int, stride: int):
        from ..coder import BaselineEncodeSession

        return BaselineEncodeSession(self.ctx, self.bits[:S], mode=self.mode, block_size=self.block_size,
                                     max_tokens=budget, stats=self.stats, payload_stride=stride)

    def _range_error(self, msgs) -> str:
        return f"messages {msgs}: a logits row the {self.mode} coder cannot code (NaN, inf or a bin without a token)"

    def _key_extra(self, sess) -> tuple:
        return _layout_key(sess.nbits, sess.out_token, sess.spec.table)


class BaselineSlotDecoder(SlotSampler):
    """:class:`SlotSampler`'s loop over a baseline decoder (``coder.BaselineDecodeStreamsSession``): a message's end is
    known on the host from its token count, every slot reads the token at its own index from its device token row
    (no host read in the loop), and every message has its own context.  ``run()`` returns each message's decoded
    bits; a token outside the code raises :class:`DecodeDivergenceError` (the repairing decode is
    ``HipArithmeticLM.decode_baseline_repair``)."""

    def __init__(self, provider, ctx, token_lists, contexts, *, mode: str, block_size: int, slots: int,
                 use_graph: bool, check_every: int = 16, compact: bool = True, share: bool = True,
                 share_prefixes: bool = True):
        n = len(token_lists)
        super().__init__(provider, ctx, contexts, [len(t) for t in token_lists], None, [0] * n, [0] * n, slots=slots,
                         use_graph=use_graph, stats=False, check_every=check_every, compact=compact, share=share,
                         share_prefixes=share_prefixes)
        self.lists = token_lists
        self.mode, self.block_size = mode, int(block_size)

    def _session(self, S: int, budget: int, Lmax: int):
        from ..coder import BaselineDecodeStreamsSession

        return BaselineDecodeStreamsSession(self.ctx, S, max_tokens=Lmax, mode=self.mode, block_size=self.block_size,
                                            rank_export=False)

    def _harvest(self, sess, fin, nl, ev, side, msgs):
        from ..codec.errors import ArithmeticRangeError, DecodeDivergenceError
        from ..coder import _bit_rows_to_lists

        if ev is not None:
            st, ob = _rows_after(ev, side, sess.state, fin), _rows_after(ev, side, sess.out_bits, fin)
            f = _state_fields(st)
            got, flags = _bit_rows_to_lists(ob, f["bit_pos"]), f["flags"]
        else:
            got, _, flags, _ = sess.harvest(fin)
        bad = msgs[(flags & _lib.NS_ST_ERR_RANGE) != 0]
        if bad.size:
            raise ArithmeticRangeError(f"messages {bad.tolist()[:8]}: a logits row the {self.mode} coder cannot code")
        bad = msgs[(flags & _lib.NS_ST_ERR_DIVERGE) != 0]
        if bad.size:
            raise DecodeDivergenceError(f"messages {bad.tolist()[:8]}: received token outside the {self.mode} code")
        return got, None

    def _key(self, sess) -> tuple:
        return _layout_key(sess.state, sess.tokmat, sess.nlen, sess.out_bits, sess.counts, sess.out_token,
                           sess.spec.table)

    def _load(self, sess, slots, msgs, nl) -> None:
        sess.load_slots(slots, [self.lists[m] for m in msgs])
