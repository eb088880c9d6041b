"""``HipArithmeticLM``: the drop-in provider behind the reference's plugin protocol.

Implements ``src/neuralstego/api.py:42-56`` (``LMProvider``: ``encode_arithmetic`` / ``decode_arithmetic`` /
``encode_seed``) plus the optional ``drain_states`` / ``load_states`` side channel probed by
``api.encode_text``/``decode_text`` (``api.py:850-854,996-1000``), mirroring ``ArithmeticLM``
(``src/neuralstego/lm/arithmetic.py:144-264``).  Unlike the reference provider (a fixed-width rank coder
that re-runs the whole context per token, ``codec/arithmetic.py:122-231``), this one runs the TRUE arithmetic
coder of ``code_base/arithmetic.py`` on the HIP kernel, batched over streams, with a KV-cached GPT-2.

Bits cross the boundary as LSB-first bit lists (``api.py:153-157``); ``encode_arithmetic`` returns token
ids; ``decode_arithmetic`` returns exactly the number of bits that were encoded (the count travels in the
state side channel as ``residual_bits`` = 8-byte big-endian bit count, the reference's CodecState format).
"""

from __future__ import annotations

from collections import deque
from typing import Deque, Dict, Iterable, List, Mapping, Optional, Sequence

from ..coder import (CoderContext, CoderParams, DecodeSession, EncodeSession, SampleSession, StreamQuality,
                     StreamingDecodeSession)
from ..exceptions import ConfigurationError

CodecState = Dict[str, object]


def coder_params_from_quality(quality: Optional[Mapping[str, object]], vocab: int, logits_dtype: str,
                              banned: Optional[Sequence[int]] = None) -> CoderParams:
    """Map the api quality dict to coder parameters.

    Keys and defaults follow ``encode_arithmetic``'s signature (``code_base/arithmetic.py:78-88``) and the
    api's key aliases (``api.py:130-141``): temp/temperature (1.0), precision (16), topk/top_k (50000)."""
    q = dict(quality or {})

    def pick(*names, default=None):
        for n in names:
            if n in q and q[n] is not None:
                return q[n]
        return default

    temp = float(pick("temp", "temperature", default=1.0))
    precision = int(pick("precision", default=16))
    # top-k aliases: the LAST one in the mapping wins, as the reference's key loop does
    # (src/neuralstego/lm/arithmetic.py:77-95) -- api.stego_encode merges {**_DEFAULT_QUALITY, **user}, so a
    # caller's (or a regeneration attempt's) "top_k" follows the default "topk" and must override it
    topk = 50000
    for key, value in q.items():
        if value is not None and key.replace("-", "_").lower() in ("topk", "top_k"):
            topk = int(value)
    if temp <= 0:
        raise ConfigurationError("temperature must be positive")
    return CoderParams(vocab=vocab, precision=precision, temp=temp, topk=topk, dtype=logits_dtype, banned=banned)


def _bits_count_state(nbits: int) -> CodecState:
    return {"history": (), "residual_bits": int(nbits).to_bytes(8, byteorder="big", signed=False)}


class ByteTokenizer:
    """Tokenizer stand-in for random-init models (no vocabulary files offline): ids = UTF-8 bytes and
    ``<|endoftext|>`` = the last id of the vocabulary (50256 for GPT-2)."""

    def __init__(self, vocab: int = 50257):
        if vocab < 257:
            raise ConfigurationError("ByteTokenizer needs a vocabulary of at least 257 ids")
        self.eos_id = vocab - 1

    def encode(self, text: str, add_special_tokens: bool = False) -> List[int]:
        _ = add_special_tokens
        if text == "<|endoftext|>":
            return [self.eos_id]
        return list(text.encode("utf-8"))

    def decode(self, ids: Iterable[int]) -> str:
        return bytes(int(i) % 256 for i in ids).decode("utf-8", errors="ignore")


CTX_CACHE_SIZE = 4  # live coder contexts per provider (distinct quality settings)


class _StopCheck:
    """The reference's per-token stop test ``stop_text in enc.decode(output)`` (``code_base/arithmetic.py:
    207-210``) without a host round trip per token.  A new occurrence of ``stop_text`` must end inside the newest
    token, so that token's text contains the last character of ``stop_text``; a per-id device table of such
    tokens is gathered by the emitted tokens inside the step (graph-capturable), and the host reads one flag
    per step and decodes 16-token tails only for the flagged streams."""

    def __init__(self, provider, sess, stop_text: str):
        import torch

        self.sess, self.stop_text, self.tok = sess, stop_text, provider.tokenizer
        self.table = provider.stop_table(stop_text)
        self.hit = torch.zeros(sess.B, dtype=torch.bool, device=sess.state.device)
        self.any = torch.zeros(1, dtype=torch.bool, device=sess.state.device)
        self.any_host = torch.zeros(1, dtype=torch.bool).pin_memory()

    def flag(self, tok) -> None:
        import torch

        live = (self.sess.state.view(torch.int32)[:, 7] & 1) == 0
        torch.logical_and(self.table.index_select(0, tok.long()), live, out=self.hit)
        torch.any(self.hit, dim=0, keepdim=True, out=self.any)

    def check(self) -> None:
        import torch

        self.any_host.copy_(self.any, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if not bool(self.any_host[0]):
            return
        cand = torch.nonzero(self.hit).flatten().cpu().tolist()
        n = self.sess.fields()["ntokens"]
        stop = []
        for i in cand:
            k = int(n[i])
            tail = self.sess.hist[i, max(0, k - 16):k].cpu().tolist()
            if self.stop_text in self.tok.decode(tail):
                stop.append(i)
        if stop:
            self.sess.mark_done(stop)


class HipArithmeticLM:
    """Arithmetic-coding provider: batched GPT-2 on PyTorch-ROCm + the HIP coder step."""

    decodes_without_state = True  # the interval coder needs no per-token history (unlike the rank coder)
    skip_done = True  # finished streams skip their attention (encode: done flag, decode: stop position; A/B, tests)
    slot_compaction = True  # native slot loops: compact the live slots once the queue is drained (off: tests that
                            # read per-step logits by row)
    share_contexts = True  # ``contexts=``: messages with equal contexts share the context's KV pages (off: A/B, tests)
    # ``qualities=``: messages whose top-k is beyond the single-pass limit run as one mixed batch on the wide kernels
    # (off: one call per distinct such quality -- A/B, tests)
    mix_wide_qualities = True
    # ``contexts=``: different contexts share the pages of a common prefix, in 64-token blocks (native
    # path, fp16 pages and share_contexts on -- with an fp8 cache the call behaves as without it)
    share_prefixes = True

    def __init__(self, model, tokenizer=None, *, device: Optional[str] = None, logits_dtype: str = "f32",
                 compute_dtype=None, banned: Optional[Sequence[int]] = None, max_batch: int = 4096,
                 kv_dtype: str = "fp16", attention_window: int = 0, logit_scale: float = 1.0):
        import torch

        from .gpt2 import BatchedGPT2

        if not torch.cuda.is_available():
            from .._lib import NativeLibraryError

            raise NativeLibraryError("HipArithmeticLM needs a ROCm GPU (the coder has no CPU path)")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        ldt = torch.float16 if logits_dtype == "f16" else torch.float32
        lm = BatchedGPT2(model, device=dev, compute_dtype=compute_dtype, logits_dtype=ldt, kv_dtype=kv_dtype,
                         logit_scale=logit_scale)
        if attention_window:
            if not lm.native:
                raise ConfigurationError("an attention window needs the native fp16 decode step on the GPU")
            if int(attention_window) < 1:
                raise ConfigurationError("attention_window must be positive (0 = unbounded)")
            lm.window = int(attention_window)
        self._init(lm, tokenizer, dev, logits_dtype, banned, max_batch)

    @classmethod
    def from_batched(cls, batched_lm, tokenizer=None, *, logits_dtype: str = "f32",
                     banned: Optional[Sequence[int]] = None, max_batch: int = 4096) -> "HipArithmeticLM":
        """Provider over any batched-logits LM with the ``prefill(context, B, max_new)`` / ``step(tokens)``
        protocol (e.g. :class:`~neuralsteganography_amd.synthetic.SyntheticBatchedLM`)."""
        import torch

        if not torch.cuda.is_available():
            from .._lib import NativeLibraryError

            raise NativeLibraryError("HipArithmeticLM needs a ROCm GPU (the coder has no CPU path)")
        self = cls.__new__(cls)
        self._init(batched_lm, tokenizer, torch.device("cuda", torch.cuda.current_device()), logits_dtype, banned,
                   max_batch)
        return self

    def _init(self, lm, tokenizer, dev, logits_dtype, banned, max_batch) -> None:
        self.lm = lm
        self.vocab = self.lm.shape.vocab
        self.tokenizer = tokenizer if tokenizer is not None else ByteTokenizer(self.vocab)
        self.logits_dtype = logits_dtype
        self.banned = list(banned) if banned is not None else None
        self.max_batch = int(max_batch)
        self.device = dev
        self._ctx_cache: Dict[tuple, CoderContext] = {}
        self._sent_end = None
        self._encode_states: List[CodecState] = []
        self._decode_states: Deque[CodecState] = deque()

    # ---------------------------------------------------------------- plumbing
    def _coder(self, params: CoderParams, B: int, mixed: bool = False) -> CoderContext:
        """Coder context for ``params`` serving batches up to ``B``.  Keyed on the parameters only (the kernels
        take B per call): a context built for a larger batch serves every smaller one, a larger B replaces it,
        and at most ``CTX_CACHE_SIZE`` parameter sets stay alive (least recently used closed first) -- each
        wide-path context holds 2*B*V*8 bytes of sort keys.  ``mixed``: the context of a call with per-message
        qualities (``params.topk`` is its ``k_max``), whose steps read temperature and precision from the table."""
        key = (params.vocab, params.precision, params.temp, params.topk, params.dtype,
               tuple(params.banned_ids()))
        if mixed:
            key = (params.vocab, params.dtype, tuple(params.banned_ids()), params.topk, "mixed")
        ctx = self._ctx_cache.pop(key, None)
        if ctx is not None and (ctx.max_batch < B or ctx.params.precision < params.precision):
            ctx.close()
            ctx = None
        if ctx is None:
            ctx = CoderContext(params, max_batch=max(B, 1), device=self.device.index)
        self._ctx_cache[key] = ctx  # re-inserted last: dict order is the LRU order
        while len(self._ctx_cache) > CTX_CACHE_SIZE:
            old = next(iter(self._ctx_cache))
            self._ctx_cache.pop(old).close()
        return ctx

    def sentence_end_table(self):
        """Per-id table of sentence-ending tokens: ``'.' in t or '!' in t or '?' in t`` for the decoded
        text of each id (``code_base/utils.py:55-57``)."""
        if self._sent_end is None:
            import numpy as np

            tab = np.zeros(self.vocab, dtype=np.uint8)
            for i in range(self.vocab):
                try:
                    txt = self.tokenizer.decode([i])
                except Exception:
                    continue
                if "." in txt or "!" in txt or "?" in txt:
                    tab[i] = 1
            self._sent_end = tab
        return self._sent_end

    def stop_table(self, stop_text: str):
        """Device bool table [vocab]: the id's decoded text contains the last character of ``stop_text``
        (only such a token can complete a new occurrence).  Cached per stop text."""
        import torch

        cache = self.__dict__.setdefault("_stop_tables", {})
        tab = cache.get(stop_text)
        if tab is None:
            host = torch.from_numpy(stop_candidates(self.tokenizer, self.vocab, stop_text))
            tab = cache[stop_text] = host.to(self.device)
        return tab

    # ---------------------------------------------------------------- protocol
    def encode_seed(self, text: str) -> List[int]:
        """``<|endoftext|>`` + tokens of ``text`` (``src/neuralstego/lm/arithmetic.py:143-160``)."""
        tok = self.tokenizer
        try:
            bos = list(tok.encode("<|endoftext|>", add_special_tokens=False))
        except TypeError:
            bos = list(tok.encode("<|endoftext|>"))
        try:
            body = list(tok.encode(text, add_special_tokens=False))
        except TypeError:
            body = list(tok.encode(text))
        return [int(t) for t in bos + body]

    def encode_arithmetic(self, bits: List[int], context: List[int], *, quality: Mapping[str, object]) -> List[int]:
        toks = self.encode_batch([bits], context, quality=quality if quality is not None else {})[0]
        return toks

    def decode_arithmetic(self, tokens: List[int], context: List[int], *, quality: Mapping[str, object]) -> List[int]:
        state = self._decode_states.popleft() if self._decode_states else None
        if not tokens:
            return []
        nbits = None
        if state is not None and state.get("residual_bits"):
            nbits = int.from_bytes(bytes(state["residual_bits"]), byteorder="big", signed=False)
        out = self.decode_batch([tokens], context, quality=quality if quality is not None else {})[0]
        return out[:nbits] if nbits is not None else out

    def drain_states(self) -> List[CodecState]:
        states = [dict(s) for s in self._encode_states]
        self._encode_states.clear()
        return states

    def load_states(self, states: Iterable[CodecState]) -> None:
        self._decode_states = deque(dict(s) for s in states)

    # ---------------------------------------------------------------- batched entry points
    def encode_batch(self, bit_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                     contexts: Optional[Sequence[Sequence[int]]] = None,
                     quality: Optional[Mapping[str, object]] = None,
                     qualities: Optional[Sequence[Mapping[str, object]]] = None, check_every: int = 16,
                     stall_steps: int = 4096, return_stats: bool = False, stop_text: Optional[str] = None,
                     graphs: Optional[bool] = None, slots: Optional[int] = None):
        """Encode independent bit lists (one GPT-2 forward + one coder launch per token for every live stream).

        On the native GPU model (the product path) the messages run through ``slots`` slots (default
        ``min(len(bit_lists), max_batch)``, :class:`~neuralsteganography_amd.lm.slots.SlotEncoder`): a finished
        message's slot takes the next queued one, KV pages follow the live tokens (``lm/kvpages.py``), the youngest
        messages are re-queued when the device is full, and the live slots are compacted once the queue is drained.
        A message's tokens do not depend on its slot or neighbours (batch-invariant decode step).  Other LMs (the
        PyTorch fp32 forward, synthetic rows) run the lockstep loop below.

        Exactly one of ``context`` (shared by every message) and ``contexts`` (one per message, e.g. one seed text
        per conversation) is given.  With ``contexts`` a message's context is prefilled into its slot's own KV pages
        when it is admitted (``BatchedGPT2.prefill_contexts``); its tokens equal
        ``encode_batch([bits], contexts[m])[0]`` -- the receiver decodes it alone with that context.  Messages whose
        contexts are equal share the context's KV pages and one prefill (``share_contexts``, ``lm/kvpages.py``);
        different contexts that begin with the same 64-token blocks share the pages and the prefill of that beginning
        (``share_prefixes``; fp16 pages only -- with ``kv_dtype="fp8"`` the call behaves as without it).
        All-equal ``contexts`` take the shared-context path; non-native LMs run their lockstep loop once per distinct
        context.

        Exactly one of ``quality`` (shared) and ``qualities`` (one per message: its own temperature, top-k and
        precision, as each ``stego_encode`` call of the reference has its own ``quality``) is given.  The coder step
        then reads every stream's values from its row of a device table (``ns_set_stream_quality``), so the messages
        still run as ONE batch; message ``m``'s tokens equal ``encode_batch([bits], ..., quality=qualities[m])[0]``.
        ``finish_sent`` is a flag of the whole step and must agree across the call.  All-equal ``qualities`` take the
        ``quality`` path.  Messages whose top-k exceeds the single-pass limit (``ns_max_topk``; the api default,
        top-k 50,000, is one) run as ONE more mixed batch on the wide kernels (``ns_set_stream_quality_wide``), so a
        call has at most two groups -- at or below the limit, and beyond it -- with the results back in the caller's
        order (``last_schedule["quality_groups"]``).  With ``mix_wide_qualities = False`` every distinct quality
        beyond the limit runs as a call of its own instead (the same tokens).

        With ``graphs`` (default) the native model's per-token step is captured once as a hipGraph and replayed,
        which removes the per-launch host cost (it dominates at small batch, and at B = 4096 it keeps the GPU busy
        across the host checks).  Non-native models ignore ``graphs``: their lockstep loop runs eagerly, and its token
        history starts at the KV budget and grows at the host checks.

        The reference coder has no underflow handling: when the interval straddles the midpoint and one
        token takes the whole range, no bit is ever fixed and ``code_base/arithmetic.py:114`` loops
        forever.  Here a stream that fixes no payload bit for ``stall_steps`` tokens raises
        :class:`ArithmeticRangeError` instead of hanging."""
        B = len(bit_lists)
        context, contexts = _one_or_many(context, contexts, B)
        quality, plist = self._quality_or_many(quality, qualities, B)
        if B == 0:
            return []
        kw = dict(check_every=check_every, stall_steps=stall_steps, return_stats=return_stats, stop_text=stop_text,
                  graphs=graphs, slots=slots)
        groups = _quality_groups(plist, self._single_pass_limit(), self.mix_wide_qualities) \
            if plist is not None else None
        if groups is not None and len(groups) > 1:
            n_enc, n_dec = len(self._encode_states), len(self._decode_states)
            res = self._by_group(self.encode_batch, bit_lists, groups, context, contexts, qualities, return_stats, **kw)
            self._requeue_states(n_enc, n_dec, bit_lists)
            self.last_schedule = dict(getattr(self, "last_schedule", None) or {}, quality_groups=len(groups))
            return res
        if contexts is not None and not getattr(self.lm, "native", False):
            n_enc, n_dec = len(self._encode_states), len(self._decode_states)
            res = self._by_context(self.encode_batch, bit_lists, contexts, return_stats, qualities=qualities,
                                   quality=quality, **kw)
            self._requeue_states(n_enc, n_dec, bit_lists)
            return res
        sq = StreamQuality(plist) if plist is not None else None  # per-message rows: one mixed batch
        params = sq.context_params() if sq is not None else \
            coder_params_from_quality(quality, self.vocab, self.logits_dtype, self.banned)
        finish = bool(dict((qualities[0] if sq is not None else quality) or {}).get("finish_sent", False))
        max_bits = max(len(b) for b in bit_lists)
        budget = 2 * max_bits + 64            # initial KV/history capacity (grows on demand)
        hard_cap = 64 * max_bits + 4096       # a stream fixing < 1/64 bit per token is reported, not looped
        if graphs is None:
            graphs = True
        if getattr(self.lm, "native", False):
            from .slots import SlotEncoder

            S = max(1, min(B, int(slots) if slots else self.max_batch))
            ctx = self._coder(params, S, mixed=sq is not None)
            if finish:
                ctx.set_sentence_end(self.sentence_end_table())
            enc = SlotEncoder(self, ctx, bit_lists, context, slots=S, finish=finish, stop_text=stop_text,
                              stats=return_stats, check_every=check_every, stall_steps=stall_steps, hard_cap=hard_cap,
                              use_graph=bool(graphs), compact=self.slot_compaction, contexts=contexts,
                              share=self.share_contexts, qualities=sq, share_prefixes=self.share_prefixes)
            toks, st = enc.run()
            self.last_schedule = {"slots": S, "evictions": enc.evictions, "compactions": enc.compactions,
                                  "max_live": enc.max_live, "kv_pages_peak": enc.kv_peak,
                                  "prefill_rows": enc.prefill_rows, "prefill_groups": enc.prefill_groups,
                                  "prefill_shared": enc.prefill_shared, "quality_groups": 1}
            if enc.prefix_entries:  # (the key set stays as it was when no prefix is shared)
                self.last_schedule.update(prefix_rows_saved=enc.prefix_rows_saved, prefix_entries=enc.prefix_entries)
            for b in bit_lists:
                sc = _bits_count_state(len(b))
                self._encode_states.append(sc)
                self._decode_states.append(dict(sc))
            return (toks, st) if return_stats else toks
        ctx = self._coder(params, B, mixed=sq is not None)
        if finish:
            ctx.set_sentence_end(self.sentence_end_table())
        logits = self.lm.prefill(context, B, budget)
        # token history: starts at the KV budget and grows at the host checks (the 64x hard cap up front would be
        # 8.6 GB at B = 4096)
        sess = EncodeSession(ctx, bit_lists, max_tokens=budget, stats=return_stats, quality=sq)
        stop = _StopCheck(self, sess, stop_text) if stop_text is not None else None

        def coder_step(lg):
            tok = sess.step(lg, finish_sent=finish)
            if stop is not None:
                stop.flag(tok)  # device-side: did any live stream emit a token that can complete stop_text?
            return tok

        toks = self._encode_loop(sess, coder_step, logits, stop, bit_lists, check_every, stall_steps, hard_cap)
        for b in bit_lists:
            st = _bits_count_state(len(b))
            self._encode_states.append(st)
            self._decode_states.append(dict(st))
        if return_stats:
            return toks, sess.stats()
        return toks

    def _encode_loop(self, sess, coder_step, logits, stop, bit_lists, check_every, stall_steps, hard_cap):
        """The eager lockstep loop of the non-native models: every stream steps until all are done."""
        B = sess.B
        t = 0
        last_pos = None
        last_move = 0
        while True:
            if stop is not None and t > 0:
                stop.check()  # code_base/arithmetic.py:207-210 ('<eos>' in run_single.py's message->bits mode)
            if t % check_every == 0:
                f = sess.fields()
                if bool((f["flags"] & 1).all()):
                    break
                sess.ensure_history(check_every + 1)
                pos = f["bit_pos"].copy()
                if last_pos is None or (pos != last_pos).any():
                    last_pos, last_move = pos, t
                if t - last_move >= stall_steps or t >= hard_cap:
                    from ..codec.errors import ArithmeticRangeError

                    stuck = [i for i in range(B) if not (f["flags"][i] & 1)]
                    if all(f["bit_pos"][i] >= len(bit_lists[i]) for i in stuck):
                        raise ArithmeticRangeError(
                            f"finish_sent: streams {stuck[:8]} produced no sentence-ending token in "
                            f"{t - last_move} tokens (the reference would keep generating forever)")
                    raise ArithmeticRangeError(
                        f"streams {stuck[:8]} fixed no payload bit for {t - last_move} tokens: the interval "
                        "straddles the midpoint and one token takes the whole range (the reference coder "
                        "has no underflow handling and would loop forever)")
            tok = coder_step(logits)
            logits = self.lm.step(tok)
            t += 1
        return sess.tokens()

    def decode_batch(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                     contexts: Optional[Sequence[Sequence[int]]] = None,
                     quality: Optional[Mapping[str, object]] = None,
                     qualities: Optional[Sequence[Mapping[str, object]]] = None, graphs: Optional[bool] = None,
                     slots: Optional[int] = None, chunk: int = 1) -> List[List[int]]:
        """Decode token lists (ragged); returns every emitted bit (callers truncate).  On the native GPU model the
        lists run through ``slots`` slots (:class:`~neuralsteganography_amd.lm.slots.SlotDecoder`, longest first,
        a message's pages mapped when it is admitted); with ``graphs`` the per-token step (coder + GPT-2 decode) is a
        replayed hipGraph, as in :meth:`encode_batch`.  Non-native models ignore ``graphs`` (eager lockstep loop).
        ``context`` / ``contexts`` as in :meth:`encode_batch`: one shared context, or one per token list; ``quality``
        / ``qualities`` likewise (one mixed batch at or below the single-pass limit and one beyond it,
        ``last_decode_schedule["quality_groups"]``; ``mix_wide_qualities = False``: one call per distinct quality
        beyond the limit).
        ``chunk`` = C in 2..16 (native model, no attention window; default 1 = one token per step): every cover token
        is known before the first step, so a slot's next C tokens go through the LM in ONE forward
        (``SlotDecoder.run_chunk``; its K/V pages are read once per C tokens) and only the coder runs token by token --
        the same bits.  The slot count is then ``min(B, max(1, slots // C))``: a forward has at most ``slots`` rows,
        so activations and logits take no more memory than ``slots`` was sized for."""
        from ..codec.errors import DecodeDivergenceError
        from .slots import check_chunk

        chunk = check_chunk(chunk)
        if chunk > 1 and (not getattr(self.lm, "native", False) or getattr(self.lm, "window", 0) > 0):
            raise ValueError("chunk > 1 needs the native HIP step without an attention window")
        B = len(token_lists)
        context, contexts = _one_or_many(context, contexts, B)
        quality, plist = self._quality_or_many(quality, qualities, B)
        if B == 0:
            return []
        groups = _quality_groups(plist, self._single_pass_limit(), self.mix_wide_qualities) \
            if plist is not None else None
        if groups is not None and len(groups) > 1:
            res = self._by_group(self.decode_batch, token_lists, groups, context, contexts, qualities, False,
                                 graphs=graphs, slots=slots, chunk=chunk)
            self.last_decode_schedule = dict(getattr(self, "last_decode_schedule", None) or {},
                                             quality_groups=len(groups))
            return res
        if contexts is not None and not getattr(self.lm, "native", False):
            return self._by_context(self.decode_batch, token_lists, contexts, False, qualities=qualities,
                                    quality=quality, graphs=graphs, slots=slots)
        for tl in token_lists:  # received ids feed the embedding gather: validate on the host first
            if any((int(t) < 0 or int(t) >= self.vocab) for t in tl):
                raise DecodeDivergenceError(f"received token id outside [0, {self.vocab})")
        sq = StreamQuality(plist) if plist is not None else None  # per-message rows: one mixed batch
        params = sq.context_params() if sq is not None else \
            coder_params_from_quality(quality, self.vocab, self.logits_dtype, self.banned)
        if graphs is None:
            graphs = True
        if getattr(self.lm, "native", False):  # the product path: slots, pages mapped at admission (lm/slots.py)
            from .slots import SlotDecoder

            S = max(1, min(B, int(slots) if slots else self.max_batch))
            # chunk > 1: the slot rule min(B, max(1, slots // chunk)) applies to the caller's slots, not to min(B, slots)
            dec = SlotDecoder(self, self._coder(params, S, mixed=sq is not None), token_lists, context,
                              slots=S if chunk == 1 else (int(slots) if slots else self.max_batch),
                              use_graph=bool(graphs), compact=self.slot_compaction, contexts=contexts,
                              share=self.share_contexts, qualities=sq, share_prefixes=self.share_prefixes,
                              chunk=chunk, check_every=max(1, 16 // chunk))  # a host check about every 16 tokens
            out = dec.run()
            self.last_decode_schedule = {"slots": dec.S, "chunk": chunk, "evictions": dec.evictions, "compactions": dec.compactions,
                                         "prefill_rows": dec.prefill_rows, "prefill_groups": dec.prefill_groups,
                                         "prefill_shared": dec.prefill_shared, "quality_groups": 1}
            if dec.prefix_entries:
                self.last_decode_schedule.update(prefix_rows_saved=dec.prefix_rows_saved,
                                                 prefix_entries=dec.prefix_entries)
            return out
        ctx = self._coder(params, B, mixed=sq is not None)
        sess = DecodeSession(ctx, token_lists, quality=sq)
        logits = self.lm.prefill(context, B, max(sess.T, 1) + 1)
        for t in range(sess.T):
            sess.step(logits)
            if t + 1 < sess.T:
                logits = self.lm.step(sess.tok[t])
        return sess.bits()

    def _by_context(self, entry, items, contexts, with_stats: bool, qualities=None, quality=None, **kw):
        """Non-native LMs: ``entry`` (``encode_batch`` / ``decode_batch``) once per distinct context over that
        context's messages (each with its own quality when ``qualities`` is given), results back in the caller's
        order."""
        groups: Dict[tuple, List[int]] = {}
        for i, c in enumerate(contexts):
            groups.setdefault(tuple(c), []).append(i)
        out: List[object] = [None] * len(items)
        stats: List[object] = [None] * len(items)
        for c, members in groups.items():
            qkw = {"quality": quality} if qualities is None else {"qualities": [qualities[i] for i in members]}
            res = entry([items[i] for i in members], list(c), **qkw, **kw)
            res, st = res if with_stats else (res, None)
            for j, i in enumerate(members):
                out[i] = res[j]
                if st is not None:
                    stats[i] = st[j]
        return (out, stats) if with_stats else out

    def _by_group(self, entry, items, groups, context, contexts, qualities, with_stats: bool, **kw):
        """``entry`` once per quality group (:func:`_quality_groups`), each over its members with their own
        contexts and qualities, results back in the caller's order."""
        out: List[object] = [None] * len(items)
        stats: List[object] = [None] * len(items)
        for members in groups:
            ckw = {"context": context} if contexts is None else {"contexts": [contexts[i] for i in members]}
            res = entry([items[i] for i in members], **ckw, qualities=[qualities[i] for i in members], **kw)
            res, st = res if with_stats else (res, None)
            for j, i in enumerate(members):
                out[i] = res[j]
                if st is not None:
                    stats[i] = st[j]
        return (out, stats) if with_stats else out

    def _requeue_states(self, n_enc: int, n_dec: int, bit_lists) -> None:
        """After an encode that ran group by group (each group queued its bit counts): the states queued since
        (``n_enc``, ``n_dec``) again, in the caller's order."""
        del self._encode_states[n_enc:]
        while len(self._decode_states) > n_dec:
            self._decode_states.pop()
        for b in bit_lists:
            sc = _bits_count_state(len(b))
            self._encode_states.append(sc)
            self._decode_states.append(dict(sc))

    def _single_pass_limit(self) -> int:
        from .. import _lib

        return _lib.max_topk(CoderParams(vocab=self.vocab, dtype=self.logits_dtype).dtype_code)

    def _quality_or_many(self, quality, qualities, n: int):
        """``(quality, None)`` for one shared quality, ``(None, params)`` -- one :class:`CoderParams` per message --
        for ``qualities``; all-equal ``qualities`` are a shared quality.  Exactly one of the two must be given,
        ``qualities`` one per message, and ``finish_sent`` (a flag of the whole step) must agree."""
        if (quality is None) == (qualities is None):
            raise ConfigurationError("give exactly one of quality (shared) and qualities (one per message)")
        if qualities is None:
            return quality, None
        qs = [dict(q or {}) for q in qualities]
        if len(qs) != n:
            raise ConfigurationError(f"{len(qs)} qualities for {n} messages")
        if len({bool(q.get("finish_sent", False)) for q in qs}) > 1:
            raise ConfigurationError("finish_sent must agree across the qualities of one call")
        plist = [coder_params_from_quality(q, self.vocab, self.logits_dtype, self.banned) for q in qs]
        if all(p == plist[0] for p in plist):
            return (qs[0] if qs else {}), None
        return None, plist

    def decode_counted(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                       contexts: Optional[Sequence[Sequence[int]]] = None, quality: Mapping[str, object], done=None,
                       check_every: int = 64):
        """``decode_batch`` that also records, per stream, the cumulative number of bits emitted after each
        token (the span splitter of ``text_to_spans`` needs the token at which a packet completes).  A stream
        whose token falls outside the kept top-k stops emitting (its later counts stay flat) instead of
        raising.  ``done(bits_lists, counts_lists) -> bool`` is polled every ``check_every`` tokens and ends
        the loop early once it holds.  Returns ``(bits per stream, counts per stream)``.

        Exactly one of ``context`` (shared) and ``contexts`` (one per stream, as in :meth:`decode_batch`) is given.
        With ``contexts`` the native model prefills every stream's own context into its KV pages
        (``BatchedGPT2.prefill_contexts``: equal contexts and common prefixes share pages) and the same lockstep
        loop runs; a stream's bits and counts equal those of the stream run alone with ``context=``.  A non-native
        LM runs the loop once per distinct context (``done`` then sees that context's streams only), results in the
        caller's order."""
        import numpy as np
        import torch

        from ..coder import _state_fields

        B = len(token_lists)
        context, contexts = _one_or_many(context, contexts, B)
        if B == 0:
            return [], []
        if contexts is not None and not getattr(self.lm, "native", False):
            return self._counted_by_context(self.decode_counted, token_lists, contexts, 2, quality=quality,
                                            done=done, check_every=check_every)
        for tl in token_lists:
            if any((int(t) < 0 or int(t) >= self.vocab) for t in tl):
                from ..codec.errors import DecodeDivergenceError

                raise DecodeDivergenceError(f"received token id outside [0, {self.vocab})")
        params = coder_params_from_quality(quality, self.vocab, self.logits_dtype, self.banned)
        ctx = self._coder(params, B)
        sess = DecodeSession(ctx, token_lists)
        counts = torch.zeros((max(sess.T, 1), B), dtype=torch.int64, device=sess.state.device)
        logits = self._prefill_streams(context, contexts, B, max(sess.T, 1) + 1)

        def snapshot(n):
            f = _state_fields(sess.state)
            ob = sess.out_bits.cpu().numpy()
            cn = counts[:n].cpu().numpy()
            bits = [np.unpackbits(ob[i], bitorder="little")[: int(f["bit_pos"][i])].tolist() for i in range(B)]
            return bits, [cn[: min(n, len(token_lists[i])), i].tolist() for i in range(B)]

        t = 0
        lens = np.asarray([len(tl) for tl in token_lists])
        while t < sess.T:
            sess.step(logits)
            counts[t].copy_(sess.state[:, 2])  # bit_pos after token t
            t += 1
            if t < sess.T:
                logits = self._lm_step(sess.tok[t - 1], lens > t)  # streams with a token t left to decode
            if done is not None and t % check_every == 0 and t < sess.T and done(*snapshot(t)):
                break
        return snapshot(t)


    def _lm_step(self, tokens, live):
        """``lm.step`` for the lockstep decodes, telling a native model which streams still need logits."""
        if getattr(self.lm, "native", False):
            return self.lm.step(tokens, live=live)
        return self.lm.step(tokens)

    def _prefill_streams(self, context, contexts, B: int, max_new: int):
        """First logits ``[B, ld]`` of the lockstep decodes: the shared ``context`` broadcast to ``B`` streams, or
        (native model) ``contexts[b]`` prefilled into stream ``b``'s own KV pages."""
        if contexts is None:
            return self.lm.prefill(context, B, max_new)
        import numpy as np

        self.lm.begin_slots(B, 0, max_new)
        kw = {}
        if not self.share_contexts:
            kw["shared"] = [False] * B
        elif not self.share_prefixes:
            kw["chains"] = [()] * B
        return self.lm.prefill_contexts(contexts, np.arange(B), **kw)

    def _counted_by_context(self, entry, token_lists, contexts, nres: int, **kw):
        """Non-native LMs: ``entry`` (a counted decode, returning ``nres`` per-stream lists) once per distinct
        context over that context's streams, results back in the caller's order (as :meth:`_by_context`)."""
        groups: Dict[tuple, List[int]] = {}
        for i, c in enumerate(contexts):
            groups.setdefault(tuple(c), []).append(i)
        out = [[None] * len(token_lists) for _ in range(nres)]
        for c, members in groups.items():
            res = entry([token_lists[i] for i in members], list(c), **kw)
            for k in range(nres):
                for j, i in enumerate(members):
                    out[k][i] = res[k][j]
        return tuple(out)

    def decode_tokens_repair(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                             contexts: Optional[Sequence[Sequence[int]]] = None,
                             quality: Mapping[str, object], enc=None) -> List[List[int]]:
        """Batched ``decode_arithmetic`` token loop with the reference's BPE repair (code_base/arithmetic.py
        :254-371): a received token outside the kept top-k' is repaired on the host from the kernel's
        ranked ids (:300-342, :func:`bpe_repair`), the token list is edited as the reference edits it, and
        the step is re-issued; an unrepairable token decodes as rank 0 while the LM is still fed the
        received token, exactly as the reference does.  Returns every emitted bit per stream.  ``context`` /
        ``contexts`` as in :meth:`decode_counted`."""
        return self.decode_counted_repair(token_lists, context, contexts=contexts, quality=quality, enc=enc,
                                          strict=True)[0]

    def decode_counted_repair(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                              contexts: Optional[Sequence[Sequence[int]]] = None,
                              quality: Mapping[str, object], enc=None, done=None, check_every: int = 64,
                              strict: bool = False):
        """:meth:`decode_tokens_repair` that also returns, per stream, the cumulative number of bits emitted
        after each token of the (repaired) list and the repaired token list itself -- the span splitter of
        ``texts_to_spans`` needs both when a cover text re-tokenises differently from the emitted ids.
        ``done(bits_lists, counts_lists, token_lists) -> bool`` is polled every ``check_every`` tokens and ends
        the loop early once it holds.  With ``strict`` a repaired token that still falls outside the top-k
        raises :class:`DecodeDivergenceError`; otherwise that stream stops emitting (its counts stay flat).
        Returns ``(bits per stream, counts per stream, token lists, edits)``: ``edits[b]`` lists ``(p, list)``,
        the stream's token list after each repair at position ``p`` (a repair at ``p`` changes positions >= p
        only), so a caller that learns afterwards that the stream ended at token e takes the list of the last
        repair at p <= e -- tokens decoded past e (another span's, out of context) may have been "repaired".
        ``context`` / ``contexts`` as in :meth:`decode_counted`: with one context per stream, a stream's bits, counts,
        repaired list and edits equal those of the stream run alone with ``context=``."""
        import torch

        from ..coder import _state_fields

        enc = enc if enc is not None else self.tokenizer
        lists = [[int(t) for t in tl] for tl in token_lists]
        B = len(lists)
        context, contexts = _one_or_many(context, contexts, B)
        if B == 0:
            return [], [], [], []
        if contexts is not None and not getattr(self.lm, "native", False):
            return self._counted_by_context(self.decode_counted_repair, lists, contexts, 4, quality=quality, enc=enc,
                                            done=done, check_every=check_every, strict=strict)
        for tl in lists:  # received ids feed the embedding gather: validate on the host first
            if any(not 0 <= t < self.vocab for t in tl):
                raise ConfigurationError(f"received token id outside [0, {self.vocab})")
        params = coder_params_from_quality(quality, self.vocab, self.logits_dtype, self.banned)
        ctx = self._coder(params, B)
        sess = StreamingDecodeSession(ctx, B, max_tokens=max(len(x) for x in lists) + 8)
        logits = self._prefill_streams(context, contexts, B, max(len(x) for x in lists) + 8)
        pos = [0] * B
        counts: List[List[int]] = [[] for _ in range(B)]
        edits: List[list] = [[] for _ in range(B)]
        dead = [False] * B  # non-strict: a stream whose repaired token still diverged stops here
        steps = 0
        while True:
            active = [pos[b] < len(lists[b]) and not dead[b] for b in range(B)]
            if not any(active):
                break
            tok = [lists[b][pos[b]] if active[b] else 0 for b in range(B)]
            last = [active[b] and pos[b] == len(lists[b]) - 1 for b in range(B)]
            sess.step(logits, tok, last, active)
            feed = list(tok)
            bad = sess.diverged()
            if bad:
                redo = [0] * B
                for b in bad:
                    coder_tok = repair_or_restore(enc, lists[b], pos[b], sess.ranked_ids(b), strict=strict)
                    if any(not 0 <= t < self.vocab for t in lists[b]):
                        raise ConfigurationError(f"repair produced a token id outside [0, {self.vocab})")
                    redo[b] = coder_tok
                    feed[b] = lists[b][pos[b]]  # repaired token, or the received one when unrepairable
                    edits[b].append((pos[b], list(lists[b])))
                sess.clear(bad)
                act2 = [b in bad for b in range(B)]
                last2 = [act2[b] and pos[b] == len(lists[b]) - 1 for b in range(B)]
                sess.step(logits, redo, last2, act2)
                still = sess.diverged()
                if still:
                    if strict:
                        from ..codec.errors import DecodeDivergenceError

                        raise DecodeDivergenceError(f"streams {still[:8]}: repaired token still outside the top-k")
                    sess.clear(still)
                    for b in still:
                        dead[b] = True
            bit_pos = _state_fields(sess.state)["bit_pos"]
            for b in range(B):
                if active[b] and not dead[b]:
                    counts[b].append(int(bit_pos[b]))
                    pos[b] += 1
            steps += 1
            if not any(pos[b] < len(lists[b]) and not dead[b] for b in range(B)):
                break
            if done is not None and steps % check_every == 0 and done(sess.bits(), counts, lists):
                break
            nxt = [pos[b] < len(lists[b]) and not dead[b] for b in range(B)]  # streams that decode a next token
            logits = self._lm_step(torch.tensor(feed, device=self.device, dtype=torch.long), nxt)
        return sess.bits(), counts, lists, edits

    # ---------------------------------------------------------------- fixed-block baseline coders (Huffman, bins)
    def _baseline_ctx(self, S: int, block_size: int) -> CoderContext:
        """The coder context of a baseline call (vocab, dtype and banned ids; the arithmetic quality is unused),
        after the block-size checks."""
        from ..coder import baseline_leaders

        params = CoderParams(vocab=self.vocab, precision=26, temp=1.0, topk=2, dtype=self.logits_dtype,
                             banned=self.banned)
        baseline_leaders(self.vocab, params.banned_ids(), block_size)
        return self._coder(params, S)

    def _baseline_groups(self, entry, items, contexts, nres: int, **kw):
        """Non-native LMs: ``entry`` once per distinct context, ``nres`` per-message result lists in caller order."""
        groups: Dict[tuple, List[int]] = {}
        for i, c in enumerate(contexts):
            groups.setdefault(tuple(c), []).append(i)
        out = [[None] * len(items) for _ in range(nres)]
        for c, members in groups.items():
            res = entry([items[i] for i in members], list(c), **kw)
            res = res if nres > 1 else (res,)
            for k in range(nres):
                for j, i in enumerate(members):
                    out[k][i] = res[k][j]
        return tuple(out) if nres > 1 else out[0]

    def encode_baseline_batch(self, bit_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                              contexts: Optional[Sequence[Sequence[int]]] = None, mode: str, block_size: int,
                              finish_sent: bool = False, return_stats: bool = False, slots: Optional[int] = None,
                              graphs: Optional[bool] = None, check_every: int = 16):
        """Encode bit lists with a fixed-block baseline coder: ``mode="huffman"`` (``code_base/huffman_baseline.py``)
        or ``mode="bins"`` (``code_base/block_baseline.py``), ``block_size`` bits per block (1..8).  ``context`` /
        ``contexts``, ``slots`` and ``graphs`` as in :meth:`encode_batch`: on the native model the messages run
        through the slot scheduler (:class:`~neuralsteganography_amd.lm.slots.BaselineSlotEncoder`), and a message's
        tokens and statistics equal those of its one-message call.  ``return_stats`` adds per message
        ``avg_NLL``, ``avg_KL`` and ``words_per_bit`` as the reference returns them."""
        from ..coder import BASELINE_MODES, BaselineEncodeSession

        if mode not in BASELINE_MODES:
            raise ConfigurationError(f"mode must be one of {BASELINE_MODES}")
        B = len(bit_lists)
        context, contexts = _one_or_many(context, contexts, B)
        ctx = self._baseline_ctx(max(1, min(B, int(slots) if slots else self.max_batch)), block_size)
        if B == 0:
            return ([], []) if return_stats else []
        kw = dict(mode=mode, block_size=block_size, finish_sent=finish_sent, return_stats=return_stats, slots=slots,
                  graphs=graphs, check_every=check_every)
        native = getattr(self.lm, "native", False)
        if contexts is not None and not native:
            return self._baseline_groups(self.encode_baseline_batch, bit_lists, contexts, 2 if return_stats else 1,
                                         **kw)
        if finish_sent:
            ctx.set_sentence_end(self.sentence_end_table())
        if native:
            from .slots import BaselineSlotEncoder

            S = max(1, min(B, int(slots) if slots else self.max_batch))
            enc = BaselineSlotEncoder(self, ctx, bit_lists, context, mode=mode, block_size=block_size, slots=S,
                                      finish=bool(finish_sent), stats=return_stats,
                                      use_graph=True if graphs is None else bool(graphs), check_every=check_every,
                                      compact=self.slot_compaction, contexts=contexts, share=self.share_contexts,
                                      share_prefixes=self.share_prefixes)
            toks, st = enc.run()
            self.last_schedule = {"slots": S, "evictions": enc.evictions, "compactions": enc.compactions,
                                  "max_live": enc.max_live, "kv_pages_peak": enc.kv_peak,
                                  "prefill_rows": enc.prefill_rows, "prefill_groups": enc.prefill_groups,
                                  "prefill_shared": enc.prefill_shared}
            return (toks, st) if return_stats else toks
        max_bits = max(len(b) for b in bit_lists)
        budget = 2 * max_bits + 64
        logits = self.lm.prefill(context, B, budget)
        sess = BaselineEncodeSession(ctx, bit_lists, mode=mode, block_size=block_size, max_tokens=budget,
                                     stats=return_stats)
        toks = self._encode_loop(sess, lambda lg: sess.step(lg, finish_sent=finish_sent), logits, None, bit_lists,
                                 check_every, 4096, max_bits + 4096 + 64)
        return (toks, sess.stats()) if return_stats else toks

    def decode_baseline_batch(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                              contexts: Optional[Sequence[Sequence[int]]] = None, mode: str, block_size: int,
                              slots: Optional[int] = None, graphs: Optional[bool] = None,
                              check_every: int = 16) -> List[List[int]]:
        """Decode token lists (ragged) with a baseline coder; returns every emitted bit (callers truncate to the
        payload length).  A token the coder cannot have emitted raises :class:`DecodeDivergenceError`
        (:meth:`decode_baseline_repair` runs the reference's BPE repairs instead).  On the native model the lists
        run through the slot scheduler with every slot's token read on the device
        (:class:`~neuralsteganography_amd.lm.slots.BaselineSlotDecoder`)."""
        from ..codec.errors import DecodeDivergenceError
        from ..coder import BASELINE_MODES, BaselineDecodeSession

        if mode not in BASELINE_MODES:
            raise ConfigurationError(f"mode must be one of {BASELINE_MODES}")
        B = len(token_lists)
        context, contexts = _one_or_many(context, contexts, B)
        S = max(1, min(B, int(slots) if slots else self.max_batch))
        native = getattr(self.lm, "native", False)
        ctx = self._baseline_ctx(S if native else max(B, 1), block_size)
        if B == 0:
            return []
        kw = dict(mode=mode, block_size=block_size, slots=slots, graphs=graphs, check_every=check_every)
        if contexts is not None and not native:
            return self._baseline_groups(self.decode_baseline_batch, token_lists, contexts, 1, **kw)
        for tl in token_lists:  # received ids feed the embedding gather: validate on the host first
            if any((int(t) < 0 or int(t) >= self.vocab) for t in tl):
                raise DecodeDivergenceError(f"received token id outside [0, {self.vocab})")
        if native:
            from .slots import BaselineSlotDecoder

            out: List[List[int]] = [[] for _ in range(B)]
            some = [i for i, tl in enumerate(token_lists) if len(tl)]
            if not some:
                return out
            ctxs = contexts if contexts is not None else [context] * B
            dec = BaselineSlotDecoder(self, ctx, [token_lists[i] for i in some], [ctxs[i] for i in some], mode=mode,
                                      block_size=block_size, slots=min(S, len(some)),
                                      use_graph=True if graphs is None else bool(graphs), check_every=check_every,
                                      compact=self.slot_compaction, share=self.share_contexts,
                                      share_prefixes=self.share_prefixes)
            got, _ = dec.run()
            for i, bits in zip(some, got):
                out[i] = bits
            self.last_decode_schedule = {"slots": dec.S, "evictions": dec.evictions, "compactions": dec.compactions,
                                         "prefill_rows": dec.prefill_rows, "prefill_groups": dec.prefill_groups,
                                         "prefill_shared": dec.prefill_shared}
            return out
        sess = BaselineDecodeSession(ctx, token_lists, mode=mode, block_size=block_size)
        logits = self.lm.prefill(context, B, max(sess.T, 1) + 1)
        for t in range(sess.T):
            sess.step(logits)
            if t + 1 < sess.T:
                logits = self.lm.step(sess.tok[t])
        return sess.bits()

    def decode_baseline_repair(self, token_lists: Sequence[Sequence[int]], context: Optional[Sequence[int]] = None, *,
                               contexts: Optional[Sequence[Sequence[int]]] = None, mode: str, block_size: int,
                               enc=None):
        """The token loops of ``decode_huffman`` / ``decode_block`` with the reference's BPE repairs
        (huffman_baseline.py:108-149, block_baseline.py:140-181), round-based like :meth:`decode_counted_repair`: a
        token the coder cannot have emitted diverges on the device with its state untouched, the host repairs the
        token list from the exported ids (:func:`huffman_repair` over the K ranked leaders, :func:`bins_repair` over
        every bin's token) and the step is re-issued.  An unrepairable token decodes as rank 0 (Huffman) or as the
        last bin (bins) while the LM is fed the received token, as the reference does.  Returns ``(bits per stream,
        repaired token lists)``."""
        import torch

        from ..coder import BASELINE_MODES, BaselineStreamingDecodeSession

        if mode not in BASELINE_MODES:
            raise ConfigurationError(f"mode must be one of {BASELINE_MODES}")
        enc = enc if enc is not None else self.tokenizer
        lists = [[int(t) for t in tl] for tl in token_lists]
        B = len(lists)
        context, contexts = _one_or_many(context, contexts, B)
        ctx = self._baseline_ctx(max(B, 1), block_size)
        if B == 0:
            return [], []
        if contexts is not None and not getattr(self.lm, "native", False):
            return self._baseline_groups(self.decode_baseline_repair, lists, contexts, 2, mode=mode,
                                         block_size=block_size, enc=enc)
        for tl in lists:
            if any(not 0 <= t < self.vocab for t in tl):
                raise ConfigurationError(f"received token id outside [0, {self.vocab})")
        cap = max((len(x) for x in lists), default=0) + 8
        sess = BaselineStreamingDecodeSession(ctx, B, cap, mode=mode, block_size=block_size)
        logits = self._prefill_streams(context, contexts, B, cap)
        pos = [0] * B
        last_bin = (1 << int(block_size)) - 1
        while True:
            active = [pos[b] < len(lists[b]) for b in range(B)]
            if not any(active):
                break
            tok = [lists[b][pos[b]] if active[b] else 0 for b in range(B)]
            sess.step(logits, tok, active)
            feed = list(tok)
            bad = sess.diverged()
            if bad:
                redo = [0] * B
                for b in bad:
                    ids = sess.ranked_ids(b)
                    snapshot = list(lists[b])
                    try:
                        if mode == "huffman":
                            redo[b] = huffman_repair(enc, lists[b], pos[b], ids)[0]
                        else:
                            bin_num, repaired = bins_repair(enc, lists[b], pos[b], ids)
                            redo[b] = ids[bin_num] if repaired else ids[last_bin]
                    except IndexError:  # the reference's merge reads past the end of the text and raises
                        from ..codec.errors import DecodeDivergenceError

                        lists[b][:] = snapshot
                        raise DecodeDivergenceError(f"stream {b}: BPE repair at token {pos[b]} runs past the end of "
                                                    "the text") from None
                    if any(not 0 <= t < self.vocab for t in lists[b]):
                        raise ConfigurationError(f"repair produced a token id outside [0, {self.vocab})")
                    feed[b] = lists[b][pos[b]]  # the repaired token, or the received one when unrepairable
                sess.clear(bad)
                sess.step(logits, redo, [b in bad for b in range(B)])
                if sess.diverged():
                    raise RuntimeError("a token taken from the exported ids diverged")  # cannot happen
            rng = sess.range_errors()
            if rng:
                from ..codec.errors import ArithmeticRangeError

                raise ArithmeticRangeError(f"streams {rng[:8]}: a logits row the {mode} coder cannot code")
            for b in range(B):
                if active[b]:
                    pos[b] += 1
            nxt = [pos[b] < len(lists[b]) for b in range(B)]
            if not any(nxt):
                break
            logits = self._lm_step(torch.tensor(feed, device=self.device, dtype=torch.long), nxt)
        return sess.bits(), lists

    def reveal_spans(self, id_lists: Sequence[Sequence[int]], *, context: Optional[Sequence[int]] = None,
                     contexts: Optional[Sequence[Sequence[int]]] = None,
                     quality: Optional[Mapping[str, object]] = None,
                     qualities: Optional[Sequence[Mapping[str, object]]] = None, slots: Optional[int] = None,
                     check_every: int = 16, graphs: Optional[bool] = None) -> List[List[List[int]]]:
        """The spans of many cover texts, given each text's ids after its seed: text i is cut into the spans its
        sender encoded after ``contexts[i]`` (else ``context``) with ``qualities[i]`` (else ``quality``; the merged
        quality, ``finish_sent`` included -- it may differ per text).  On the native GPU model (no attention window)
        the texts run as ONE slot-scheduled batch (:class:`~neuralsteganography_amd.lm.slots.SlotRevealer`,
        ``ns_decode_step_streams``): a slot decodes a text's remainder until its span settles, the rest is queued as
        a fresh stream, and top-k values beyond the single-pass limit form a second group on the wide kernels (at
        most two groups a call).  A text whose ids leave the kept top-k before a span settles (a cover that
        re-tokenised differently from the emitted ids) leaves the batch; such texts, and every text on another LM,
        run through the round-based code of ``cover.texts_to_spans`` with :meth:`decode_counted_repair` -- the BPE
        repair -- once per distinct quality, so a text's spans are what that path returns for it.
        ``last_reveal_schedule``: ``spans``, ``fallback_texts``, ``steps``, ``discarded_tokens`` (decoded past a
        span's end before the check that noticed it), ``evictions``, ``compactions``, ``prefill_rows``,
        ``kv_pages_peak``, ``quality_groups``."""
        from ..cover import _quality_key, _spans_by_rounds

        n = len(id_lists)
        context, contexts = _one_or_many(context, contexts, n)
        if (quality is None) == (qualities is None):
            raise ConfigurationError("give exactly one of quality (shared) and qualities (one per text)")
        qs = [dict(q or {}) for q in qualities] if qualities is not None else [dict(quality)] * n
        if len(qs) != n:
            raise ConfigurationError(f"{len(qs)} qualities for {n} texts")
        if slots is not None and int(slots) < 1:
            raise ConfigurationError("slots must be positive")
        rest = [[int(t) for t in ids] for ids in id_lists]
        for tl in rest:  # received ids feed the embedding gather: validate on the host first
            if any(not 0 <= t < self.vocab for t in tl):
                raise ConfigurationError(f"received token id outside [0, {self.vocab})")
        ctxs = contexts if contexts is not None else [list(context)] * n
        spans: List[List[List[int]]] = [[] for _ in range(n)]
        sched = dict.fromkeys(REVEAL_SCHEDULE_KEYS, 0)
        todo = [i for i in range(n) if rest[i]]
        if todo and getattr(self.lm, "native", False) and not getattr(self.lm, "window", 0):
            from .slots import SlotRevealer

            plist = [coder_params_from_quality(qs[i], self.vocab, self.logits_dtype, self.banned) for i in todo]
            finishes = [bool(qs[i].get("finish_sent")) for i in todo]
            sent_end = self.sentence_end_table() if any(finishes) else None
            groups = _quality_groups(plist, self._single_pass_limit(), mix_wide=True)
            left = []
            for members in groups:
                sq = StreamQuality([plist[j] for j in members])
                S = max(1, min(len(members), int(slots) if slots else self.max_batch))
                rev = SlotRevealer(self, self._coder(sq.context_params(), S, mixed=True),
                                   [rest[todo[j]] for j in members], [ctxs[todo[j]] for j in members], sq,
                                   [finishes[j] for j in members], sent_end, slots=S,
                                   use_graph=graphs is None or bool(graphs), labels=[todo[j] for j in members],
                                   check_every=check_every, compact=self.slot_compaction, share=self.share_contexts,
                                   share_prefixes=self.share_prefixes)
                rev.run()
                for k, j in enumerate(members):
                    spans[todo[j]] = rev.spans[k]
                    rest[todo[j]] = rev.rest[k] if k in rev.fallback else []
                left += [todo[members[k]] for k in rev.fallback]
                sched["kv_pages_peak"] = max(sched["kv_pages_peak"], rev.kv_peak)
                for key, v in (("steps", rev.steps), ("discarded_tokens", rev.discarded),
                               ("evictions", rev.evictions), ("compactions", rev.compactions),
                               ("prefill_rows", rev.prefill_rows)):
                    sched[key] += v
            sched["quality_groups"] = len(groups)
            todo = sorted(left)
        sched["fallback_texts"] = len(todo)
        by_q: Dict[str, List[int]] = {}
        for i in todo:  # the round-based path takes one quality per call
            by_q.setdefault(_quality_key(qs[i]), []).append(i)
        for members in by_q.values():
            got = _spans_by_rounds([rest[i] for i in members], [tuple(ctxs[i]) for i in members],
                                   {tuple(ctxs[i]): list(ctxs[i]) for i in members}, self, qs[members[0]],
                                   labels=members)
            for i, sp in zip(members, got):
                spans[i] = spans[i] + sp
        sched["spans"] = sum(len(s) for s in spans)
        self.last_reveal_schedule = sched
        return spans

    def sample_batch(self, B: int, length: int, context: Optional[Sequence[int]] = None, *,
                     contexts: Optional[Sequence[Sequence[int]]] = None, lengths: Optional[Sequence[int]] = None,
                     temperatures: Optional[Sequence[float]] = None, topks: Optional[Sequence[int]] = None,
                     seeds: Optional[Sequence[int]] = None, slots: Optional[int] = None,
                     graphs: Optional[bool] = None, temperature: float = 1.0, topk: int = -1, seed: int = 0,
                     stream_offset: int = 0, stats: bool = True):
        """B independent non-stego samples of ``length`` tokens from one context (code_base/sample.py, batched):
        returns ``(token lists, per-stream {avg_NLL, avg_KL, avg_Hq})``.

        With none of ``contexts``, ``lengths``, ``temperatures``, ``topks``, ``seeds``, ``slots`` and ``graphs`` the
        B streams run in lockstep from the one ``context`` (``ns_sample_step``), stream b drawing with
        ``(seed, stream_offset + b)``.

        With any of them the samples are B MESSAGES of one slot-scheduled batch (``lm/slots.py`` ``SlotSampler``,
        ``ns_sample_step_streams``): message i has its own context (``contexts[i]``, else ``context``), length
        (``lengths[i]``, else ``length``), temperature and top-k (``temperatures[i]`` / ``topks[i]``, else the
        scalars; top-k <= 0: every id) and draw key -- ``(seed, stream_offset + i)`` without ``seeds``, which makes
        the all-scalar call a special case and keeps ``stream_offset`` a shard's first stream id, and
        ``(seeds[i], stream_offset)`` with them, so message i equals ``sample_batch(1, lengths[i], contexts[i], ...,
        seed=seeds[i], stream_offset=stream_offset)``.  Through ``slots`` slots (default ``min(B, max_batch)``) a
        finished message's slot takes the next one, longest first; contexts are prefilled ragged into KV pages and
        equal contexts and common prefixes share pages as in :meth:`encode_batch`.  Top-k values beyond the
        single-pass limit (and "every id") form a second mixed group on the wide kernels, so a call has at most two
        groups (``last_sample_schedule["quality_groups"]``).  Other LMs (any ``prefill`` / ``step`` object) run the
        lockstep loop once per distinct (context, length, temperature, top-k), with the same draw keys."""
        import torch

        if all(v is None for v in (contexts, lengths, temperatures, topks, seeds, slots, graphs)):
            if context is None:
                raise ConfigurationError("give exactly one of context (shared) and contexts (one per message)")
        else:
            return self._sample_streams(int(B), length, context, contexts, lengths, temperatures, topks, seeds, slots,
                                        graphs, temperature, topk, seed, stream_offset, stats)
        params = CoderParams(vocab=self.vocab, precision=16, temp=float(temperature),
                             topk=int(topk) if int(topk) > 0 else self.vocab, dtype=self.logits_dtype,
                             banned=self.banned)
        ctx = self._coder(params, B)
        sess = SampleSession(ctx, B, seed=seed, topk=topk, temp=temperature, stream_offset=stream_offset,
                             max_tokens=max(1, length), stats=stats)
        logits = self.lm.prefill(context, B, length + 1)
        for t in range(length):
            tok = sess.step(logits)
            if t + 1 < length:
                logits = self.lm.step(tok.to(torch.long))
        return sess.tokens(), (sess.stats() if stats else None)

    def _sample_streams(self, n, length, context, contexts, lengths, temperatures, topks, seeds, slots, graphs,
                        temperature, topk, seed, stream_offset, stats):
        """:meth:`sample_batch` with per-message values: validation (before any device use), the two top-k groups,
        one :class:`SlotSampler` run per group on the native model, results back in the caller's order."""
        context, contexts = _one_or_many(context, contexts, n)
        lens, temps, tks = sample_plan(n, length, lengths, temperature, temperatures, topk, topks)
        sds, gids = sample_draw_keys(n, seeds, seed, stream_offset)
        if slots is not None and int(slots) < 1:
            raise ConfigurationError("slots must be positive")
        if n == 0:
            self.last_sample_schedule = dict.fromkeys(SAMPLE_SCHEDULE_KEYS, 0)
            return [], ([] if stats else None)
        ctxs = contexts if contexts is not None else [list(context)] * n
        groups = sample_topk_groups(tks, self._single_pass_limit())
        plist = [CoderParams(vocab=self.vocab, precision=16, temp=temps[i], topk=tks[i] if tks[i] > 0 else self.vocab,
                             dtype=self.logits_dtype, banned=self.banned) for i in range(n)]
        toks: List[object] = [None] * n
        sts: List[object] = [None] * n
        sched = dict.fromkeys(SAMPLE_SCHEDULE_KEYS, 0)
        native = getattr(self.lm, "native", False)
        for members in groups:
            sq = StreamQuality([plist[i] for i in members])
            pick = lambda xs: [xs[i] for i in members]  # noqa: E731
            if native:
                from .slots import SlotSampler

                S = max(1, min(len(members), int(slots) if slots else self.max_batch))
                smp = SlotSampler(self, self._coder(sq.context_params(), S, mixed=True), pick(ctxs), pick(lens), sq,
                                  pick(sds), pick(gids), slots=S, use_graph=graphs is None or bool(graphs),
                                  stats=stats, compact=self.slot_compaction, share=self.share_contexts,
                                  share_prefixes=self.share_prefixes)
                res, st = smp.run()
                sched["slots"] = max(sched["slots"], S)
                sched["kv_pages_peak"] = max(sched["kv_pages_peak"], smp.kv_peak)
                for k, v in (("prefill_rows", smp.prefill_rows), ("compactions", smp.compactions),
                             ("evictions", smp.evictions)):
                    sched[k] += v
            else:
                res, st = self._sample_lockstep(sq, pick(ctxs), pick(lens), pick(sds), pick(gids), stats)
            for j, i in enumerate(members):
                toks[i] = res[j]
                if st is not None:
                    sts[i] = st[j]
        sched["quality_groups"] = len(groups)
        self.last_sample_schedule = sched
        return toks, (sts if stats else None)

    def _sample_lockstep(self, sq, ctxs, lens, sds, gids, stats):
        """Non-native LMs: the lockstep loop once per distinct (context, length, temperature, top-k) over that
        group's messages, every message with its own draw key (``ns_sample_step_streams`` rows)."""
        import torch

        by: Dict[tuple, List[int]] = {}
        for i, c in enumerate(ctxs):
            q = sq.params[i]
            by.setdefault((tuple(c[-1022:]), lens[i], q.temp, q.topk), []).append(i)
        toks: List[object] = [None] * len(ctxs)
        sts: List[object] = [None] * len(ctxs)
        for (c, L, _, _), members in by.items():
            B = len(members)
            ctx = self._coder(sq.context_params(), B, mixed=True)
            sess = SampleSession(ctx, B, max_tokens=L, stats=stats, quality=sq.take(members),
                                 seeds=[sds[i] for i in members], gids=[gids[i] for i in members], lengths=[L] * B)
            logits = self.lm.prefill(list(c), B, L + 1)
            for t in range(L):
                tok = sess.step(logits)
                if t + 1 < L:
                    logits = self.lm.step(tok.to(torch.long))
            res, st = sess.tokens(), (sess.stats() if stats else None)
            for j, i in enumerate(members):
                toks[i] = res[j]
                if st is not None:
                    sts[i] = st[j]
        return toks, (sts if stats else None)


SAMPLE_SCHEDULE_KEYS = ("slots", "quality_groups", "prefill_rows", "compactions", "evictions", "kv_pages_peak")
REVEAL_SCHEDULE_KEYS = ("spans", "fallback_texts", "steps", "discarded_tokens", "evictions", "compactions",
                        "prefill_rows", "kv_pages_peak", "quality_groups")


def sample_draw_keys(n: int, seeds, seed: int, stream_offset: int):
    """``(seeds, draw ids)`` of the n messages of a ``sample_batch`` call: without ``seeds`` message i draws with
    ``(seed, stream_offset + i)`` -- the lockstep call's rule, a shard being ``stream_offset`` -- and with them with
    ``(seeds[i], stream_offset)``, what ``sample_batch(1, ..., seed=seeds[i], stream_offset=stream_offset)`` uses."""
    off = int(stream_offset)
    if seeds is None:
        return [int(seed)] * n, [off + i for i in range(n)]
    sds = [int(s) for s in seeds]
    if len(sds) != n:
        raise ConfigurationError(f"{len(sds)} seeds for {n} messages")
    return sds, [off] * n


def sample_plan(n: int, length, lengths, temperature, temperatures, topk, topks):
    """Per-message ``(lengths, temperatures, topks)`` of a ``sample_batch`` call from the lists and the scalars
    they default to; top-k as given (<= 0: every id).  A length below 1 is a ``ValueError`` (``sample.py:7`` asserts
    ``length > 0``); a list of the wrong size and a temperature that is not positive are ConfigurationErrors."""
    def many(name, values, default, conv):
        if values is None:
            return [conv(default)] * n
        out = [conv(v) for v in values]
        if len(out) != n:
            raise ConfigurationError(f"{len(out)} {name} for {n} messages")
        return out

    lens = many("lengths", lengths, length, int)
    temps = many("temperatures", temperatures, temperature, float)
    tks = many("topks", topks, topk, int)
    if any(v < 1 for v in lens):
        raise ValueError("length must be positive")  # sample.py:7 asserts length > 0
    if any(not v > 0 for v in temps):
        raise ConfigurationError("temperature must be positive")
    return lens, temps, tks


def sample_topk_groups(topks: Sequence[int], limit: int) -> List[List[int]]:
    """Message indices per slot run of a ``sample_batch`` call, grouped as :func:`_quality_groups` groups encode
    qualities with ``mix_wide``: the messages whose top-k fits the single-pass kernel in one mixed group, the others
    -- "every id" (top-k <= 0) among them, whatever the vocabulary -- in one more on the wide kernels."""
    plist = [CoderParams(vocab=2, topk=int(k) if int(k) > 0 else (1 << 30)) for k in topks]
    return _quality_groups(plist, limit, mix_wide=True)


def _quality_groups(plist: Sequence[CoderParams], limit: int, mix_wide: bool = False) -> List[List[int]]:
    """Message indices per call of a ``qualities=`` request: every message whose top-k fits the single-pass kernel
    (``limit`` = ``ns_max_topk``) in ONE mixed group, then the messages beyond it -- with ``mix_wide`` as ONE more
    mixed group (the wide kernels read per-stream rows, ``ns_set_stream_quality_wide``), else one group per distinct
    (temp, topk, precision), in order of first appearance.  The two mixed groups stay apart: the single-pass step is
    several times faster than the wide chain, which would otherwise serve the narrow messages too."""
    mixed = [i for i, p in enumerate(plist) if p.topk <= limit]
    if mix_wide:
        beyond = [i for i, p in enumerate(plist) if p.topk > limit]
        return ([mixed] if mixed else []) + ([beyond] if beyond else [])
    wide: Dict[tuple, List[int]] = {}
    for i, p in enumerate(plist):
        if p.topk > limit:
            wide.setdefault((p.temp, p.topk, p.precision), []).append(i)
    return ([mixed] if mixed else []) + list(wide.values())


def _one_or_many(context, contexts, n: int):
    """``(context, None)`` for a shared context, ``(None, contexts)`` for one context per message; equal
    ``contexts`` are a shared context.  Exactly one of the two must be given, and ``contexts`` one per message."""
    if (context is None) == (contexts is None):
        raise ConfigurationError("give exactly one of context (shared) and contexts (one per message)")
    if contexts is None:
        return context, None
    ctxs = [[int(t) for t in c] for c in contexts]
    if len(ctxs) != n:
        raise ConfigurationError(f"{len(ctxs)} contexts for {n} messages")
    if all(c == ctxs[0] for c in ctxs):
        return (ctxs[0] if ctxs else []), None
    return None, ctxs


def stop_candidates(tokenizer, vocab: int, stop_text: str):
    """Per-id bool table of the tokens that can complete a new occurrence of ``stop_text`` (the newest token of
    ``stop_text in enc.decode(output)``, ``code_base/arithmetic.py:207-210``): the id's lone text contains the
    last character of ``stop_text``.  When that character is more than one UTF-8 byte, a byte-level BPE can
    split it across tokens and the completing token's lone text is U+FFFD (``errors='replace'``) or empty
    (``errors='ignore'``): such ids -- lone text with U+FFFD, empty, or not re-encoding to the id -- are
    candidates too, and so is an id whose lone decode raises."""
    import numpy as np

    if not stop_text:
        raise ConfigurationError("stop_text must be non-empty")
    last = stop_text[-1]
    multibyte = len(last.encode("utf-8")) > 1
    tab = np.zeros(vocab, dtype=np.bool_)
    for i in range(vocab):
        try:
            txt = tokenizer.decode([i])
        except Exception:
            tab[i] = True  # undecodable alone: always check it on the host
            continue
        if last in txt:
            tab[i] = True
        elif multibyte:
            if not txt or "\ufffd" in txt:
                tab[i] = True
                continue
            try:
                try:
                    back = list(tokenizer.encode(txt, add_special_tokens=False))
                except TypeError:
                    back = list(tokenizer.encode(txt))
            except Exception:
                back = None
            tab[i] = back != [i]
    return tab


def bpe_repair(enc, inp: List[int], i: int, ranked_ids: Sequence[int]):
    """The reference's BPE repair for a received token outside the kept top-k (code_base/arithmetic.py:300-342),
    restated line for line over ``ranked_ids`` (the kernel's ranked kept ids).  Edits ``inp`` in place as the
    reference does -- including its deletion loop, which removes every other following token when more than
    one is merged -- and returns ``(token to decode, repaired?)``; unrepairable tokens decode as rank 0."""
    true_token_text = enc.decode([inp[i]])
    for cand in ranked_ids:
        cand = int(cand)
        prop_token_text = enc.decode([cand])
        if inp[i] == 128 and cand == 198:  # common case that is not caught
            inp[i] = cand
            return cand, True
        if len(prop_token_text) <= len(true_token_text) and \
                prop_token_text == true_token_text[:len(prop_token_text)]:
            suffix = true_token_text[len(prop_token_text):]
            suffix_tokens = enc.encode(suffix)
            inp[i] = cand
            inp[i + 1:i + 1] = suffix_tokens
            return cand, True
        elif len(prop_token_text) > len(true_token_text) and \
                true_token_text == prop_token_text[:len(true_token_text)]:
            whole_text = true_token_text
            num_extra = 1
            while len(whole_text) < len(prop_token_text):
                whole_text += enc.decode([inp[i + num_extra]])
                num_extra += 1
            if prop_token_text == whole_text[:len(prop_token_text)]:
                inp[i] = cand
                for j in range(1, num_extra):
                    del inp[i + j]
                if len(whole_text) > len(prop_token_text):
                    suffix = whole_text[len(prop_token_text):]
                    inp[i + 1:i + 1] = enc.encode(suffix)
                return cand, True
    return int(ranked_ids[0]), False


def repair_or_restore(enc, inp: List[int], i: int, ranked_ids: Sequence[int], *, strict: bool) -> int:
    """:func:`bpe_repair` for the batched decoder: the token the coder decodes at position ``i``.

    The reference's longer-token branch reads ``inp[i + num_extra]`` and deletes ``inp[i + j]`` as it goes; when
    the merge reaches past the end of the text that raises ``IndexError`` out of ``decode_arithmetic``
    (``code_base/arithmetic.py:321-333``) -- possibly after ``inp`` was already edited.  Here the list is restored
    to its state before the attempt (so the LM is fed the received token and later spans are cut from an unedited
    list); strict decoding raises :class:`DecodeDivergenceError` as the reference raises, the lenient span
    splitter decodes the rank-0 token as an unrepairable one."""
    snapshot = list(inp)
    try:
        return bpe_repair(enc, inp, i, ranked_ids)[0]
    except IndexError:
        inp[:] = snapshot
        if strict:
            from ..codec.errors import DecodeDivergenceError

            raise DecodeDivergenceError(f"BPE repair at token {i} runs past the end of the text") from None
        return int(ranked_ids[0])


def huffman_repair(enc, inp: List[int], i: int, ranked_ids: Sequence[int]):
    """``decode_huffman``'s BPE repair (code_base/huffman_baseline.py:108-149) over the K ranked leaders.  Line by
    line it is the arithmetic decoder's (:func:`bpe_repair`): the 128 -> 198 case (:113), the ``<=`` prefix test
    (:119), the longer-token merge with its deletion loop (:129-146), and rank 0 for an unrepairable token (:149)
    while the LM is still fed the received one.  Returns ``(token to decode, repaired?)``."""
    return bpe_repair(enc, inp, i, ranked_ids)


def bins_repair(enc, inp: List[int], i: int, bin_tokens: Sequence[int]):
    """``decode_block``'s BPE repair (code_base/block_baseline.py:140-181), restated line for line over
    ``bin_tokens`` (every bin's token in bin order, the kernel's export).  It differs from the Huffman one: the
    prefix test is strict (``<``, :154), there is no 128 -> 198 case, and the bits decoded are those of the loop
    variable ``bin_num`` -- so an unrepairable token decodes as the LAST bin (:142,183) with ``inp`` untouched.
    Edits ``inp`` in place as the reference does; returns ``(bin to decode, repaired?)``."""
    true_token_text = enc.decode([inp[i]])
    bin_num = 0
    for bin_num, cand in enumerate(bin_tokens):
        cand = int(cand)
        prop_token_text = enc.decode([cand])
        if len(prop_token_text) < len(true_token_text) and \
                prop_token_text == true_token_text[:len(prop_token_text)]:
            suffix = true_token_text[len(prop_token_text):]
            suffix_tokens = enc.encode(suffix)
            inp[i] = cand
            inp[i + 1:i + 1] = suffix_tokens
            return bin_num, True
        elif len(prop_token_text) > len(true_token_text) and \
                true_token_text == prop_token_text[:len(true_token_text)]:
            whole_text = true_token_text
            num_extra = 1
            while len(whole_text) < len(prop_token_text):
                whole_text += enc.decode([inp[i + num_extra]])
                num_extra += 1
            if prop_token_text == whole_text[:len(prop_token_text)]:
                inp[i] = cand
                for j in range(1, num_extra):
                    del inp[i + j]
                if len(whole_text) > len(prop_token_text):
                    suffix = whole_text[len(prop_token_text):]
                    inp[i + 1:i + 1] = enc.encode(suffix)
                return bin_num, True
    return bin_num, False


__all__ = ["HipArithmeticLM", "ByteTokenizer", "coder_params_from_quality", "bpe_repair", "repair_or_restore",
           "stop_candidates", "huffman_repair", "bins_repair"]
