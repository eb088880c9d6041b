"""Cover generation with the quality gate and regeneration loop (``src/neuralstego/api.py:418-705``),
batched (SURVEY §8(f) 2, config C5 "quality-guard on").

``cover_generate`` / ``cover_reveal`` keep the reference's signatures, defaults (``DEFAULT_GATE_THRESHOLDS``,
``DEFAULT_REGEN_STRATEGY``, ``api.py:89-104``), attempt schedule (``_iter_attempts``, ``:491-523``: attempt 1
uses the caller's seed and quality, later attempts pop the next seed of the pool, ``top_k`` and ``temp``
overrides), guard (``QualityGuard(LMScorer(prefer_transformers=False))`` by default, ``:118-127``) and errors
(``QualityGateError`` with the last attempt's text, reasons and metrics).

``cover_generate_batch`` runs the same schedule for MANY secrets: attempt r encodes every still-rejected
secret in ONE lockstep batch (all their packets are streams of one GPT-2 + HIP-coder loop,
``stego_encode_batch``), the guard scores all the resulting covers at once (one batched GPU forward on the
transformers branch), and only the rejected secrets go on to attempt r+1.  With ``seed_texts`` every secret has
its own seed (one conversation per recipient) and follows that seed's schedule; ``cover_reveal_batch`` and
``texts_to_spans`` take ``seed_texts`` likewise.
"""

from __future__ import annotations

import json
import logging
from collections import deque
from copy import deepcopy
from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Mapping, Optional, Sequence

from .codec.textio import seed_to_ids, spans_to_text, text_to_spans
from .detect import GuardResult, QualityGuard
from .exceptions import ConfigurationError, QualityGateError
from .metrics import LMScorer
from .stego import normalise_quality, stego_decode, stego_encode_batch

log = logging.getLogger(__name__)

DEFAULT_GATE_THRESHOLDS: Dict[str, float] = {  # api.py:89-94
    "max_ppl": 120.0,
    "max_ngram_repeat": 0.35,
    "min_ttr": 0.25,
    "max_avg_entropy": 5.5,
}

DEFAULT_REGEN_STRATEGY: Dict[str, Any] = {  # api.py:97-104 (the reference's Persian seed pool)
    "seed_pool": [
        "در یک گفت‌وگوی کوتاه درباره‌ی فناوری صحبت می‌کنیم.",
        "در یک گفت‌وگوی دوستانه درباره‌ی فرهنگ و هنر صحبت می‌کنیم.",
    ],
    "top_k_steps": [80, 70, 60],
    "temperature_steps": [0.8, 0.7],
}

_DEFAULT_GUARD: Optional[QualityGuard] = None


@dataclass
class Attempt:
    """``api.py:74-78`` ``_AttemptConfig``."""

    seed_text: str
    overrides: Dict[str, Any]
    seed_variant: str


def _ensure_guard(guard: Optional[QualityGuard]) -> QualityGuard:
    global _DEFAULT_GUARD
    if guard is not None:
        return guard
    if _DEFAULT_GUARD is None:
        _DEFAULT_GUARD = QualityGuard(lm_scorer=LMScorer(prefer_transformers=False))
    return _DEFAULT_GUARD


def prepare_gate_thresholds(overrides: Optional[Mapping[str, float]]) -> Dict[str, float]:
    """``api.py:451-465``: defaults updated by the non-None overrides (floats, else ConfigurationError)."""
    out = dict(DEFAULT_GATE_THRESHOLDS)
    for key, value in (overrides or {}).items():
        if value is None:
            continue
        try:
            out[str(key)] = float(value)
        except (TypeError, ValueError) as exc:
            raise ConfigurationError(f"invalid threshold value for {key!s}: {value!r}") from exc
    return out


def prepare_regen_strategy(strategy: Optional[Mapping[str, Any]]) -> Dict[str, Any]:
    """``api.py:468-479``."""
    merged = deepcopy(DEFAULT_REGEN_STRATEGY)
    for key, value in (strategy or {}).items():
        if value is not None:
            merged[str(key)] = value
    for key in ("seed_pool", "top_k_steps", "temperature_steps"):
        merged[key] = list(merged.get(key, []))
    return merged


def _as_int(value: Any) -> int:
    try:
        return int(value)
    except (TypeError, ValueError):
        return int(float(value))


def _as_float(value: Any) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ConfigurationError(f"invalid numeric value for regeneration strategy: {value!r}")


def iter_attempts(seed_text: str, regen_attempts: int, strategy: Optional[Mapping[str, Any]]) -> Iterable[Attempt]:
    """``api.py:496-523``: attempt 0 = the caller's seed, no overrides; attempt i > 0 = next pool seed (or the
    caller's once the pool is empty), next ``top_k`` step, next ``temp`` step."""
    cfg = prepare_regen_strategy(strategy)
    seeds = deque(str(s) for s in cfg.get("seed_pool", []))
    ks = deque(cfg.get("top_k_steps", []))
    temps = deque(cfg.get("temperature_steps", []))
    for i in range(max(regen_attempts, 0) + 1):
        if i == 0:
            yield Attempt(seed_text, {}, "base")
            continue
        seed = str(seeds.popleft()) if seeds else seed_text
        over: Dict[str, Any] = {}
        if ks:
            over["top_k"] = _as_int(ks.popleft())
        if temps:
            over["temp"] = _as_float(temps.popleft())
        yield Attempt(seed, over, f"alt-{i}")


def _normalise_secret(secret) -> bytes:
    if isinstance(secret, bytes):
        return secret
    if isinstance(secret, str):
        return secret.encode("utf-8")
    raise TypeError("secret must be bytes or string")


def _tokenizer_of(lm) -> Any:
    tok = getattr(lm, "tokenizer", None)
    if tok is None:
        raise ConfigurationError("language model tokenizer unavailable for cover rendering")
    return tok


def _ensure_cover_lm(lm):
    if lm is not None:
        return lm
    from .lm import load_lm

    try:
        return load_lm("gpt2-fa")  # api.py:391-395 default provider
    except Exception as exc:
        raise ConfigurationError("failed to load default language model") from exc


def _one_or_many_seeds(seed_text: Optional[str], seed_texts: Optional[Sequence[str]], n: int):
    """``(seed_text, None)`` for a shared seed, ``(None, seeds)`` for one seed per message (``n`` of them).  Exactly
    one of the two must be given."""
    if (seed_text is None) == (seed_texts is None):
        raise ConfigurationError("give exactly one of seed_text (shared) and seed_texts (one per message)")
    if seed_texts is None:
        return seed_text, None
    seeds = [str(s) for s in seed_texts]
    if len(seeds) != n:
        raise ConfigurationError(f"{len(seeds)} seed texts for {n} messages")
    return None, seeds


def _render_covers(payloads: Sequence[bytes], *, seed_text: Optional[str] = None,
                   seed_texts: Optional[Sequence[str]] = None, quality: Mapping[str, Any], chunk_bytes: int,
                   use_crc: bool, ecc: str, nsym: int, lm) -> List[str]:
    """``_generate_cover_once`` (``api.py:526-562``) for many payloads: one batched stego_encode.  ``seed_texts``:
    one seed per payload (equal seeds are passed on as one shared ``seed_text``), each cover rendered after its own
    seed's ids."""
    seeds = [seed_text] * len(payloads) if seed_texts is None else list(seed_texts)
    skw = {"seed_texts": seeds} if len(set(seeds)) > 1 else {"seed_text": seeds[0] if seeds else (seed_text or "")}
    results = stego_encode_batch(list(payloads), chunk_bytes=chunk_bytes, use_crc=use_crc, ecc=ecc, nsym=nsym,
                                 quality=dict(quality), lm=lm, **skw)
    tok = _tokenizer_of(lm)
    ids = {s: seed_to_ids(s, tok) for s in set(seeds)}
    return [spans_to_text([list(map(int, s)) for s in res], ids[seed], tok) for res, seed in zip(results, seeds)]


def cover_generate_batch(secrets: Sequence[Any], *, seed_text: Optional[str] = None,
                         seed_texts: Optional[Sequence[str]] = None,
                         quality: Optional[Mapping[str, object]] = None,
                         chunk_bytes: int = 256, use_crc: bool = True, ecc: str = "rs", nsym: int = 10, lm=None,
                         quality_gate: bool = True, gate_thresholds: Optional[Mapping[str, float]] = None,
                         regen_attempts: int = 2, regen_strategy: Optional[Mapping[str, Any]] = None,
                         quality_guard: Optional[QualityGuard] = None, return_errors: bool = False,
                         return_attempts: bool = False) -> List[Any]:
    """One cover text per secret.  A secret whose every attempt is rejected raises ``QualityGateError`` (the
    first such, in input order), or leaves the error in its slot with ``return_errors=True``.

    Exactly one of ``seed_text`` (shared) and ``seed_texts`` (one per secret, as each ``cover_generate`` call of the
    reference has its own seed, e.g. one conversation per recipient) is given.  Message ``i`` then follows the
    schedule of ITS seed, ``iter_attempts(seed_texts[i], ...)``: attempt 1 uses its own seed, later attempts the
    pool's seeds (equal across messages: one shared context) and, once the pool is empty, its own seed again.
    Attempt r is still one ``stego_encode_batch`` over the still-rejected messages and one ``evaluate_batch``; the
    results equal ``cover_generate(secrets[i], seed_text=seed_texts[i], ...)`` one at a time.

    ``return_attempts``: a passed slot holds ``(text, Attempt)`` -- the receiver needs the seed of the attempt that
    was accepted (``Attempt.seed_text``; ``seed_variant`` is ``"base"`` or ``"alt-<r>"``)."""
    payloads = [_normalise_secret(s) for s in secrets]
    n = len(payloads)
    seed_text, seeds = _one_or_many_seeds(seed_text, seed_texts, n)
    if seeds is None:
        seeds = [seed_text] * n
    provider = _ensure_cover_lm(lm)
    q = normalise_quality(quality)
    kw = dict(chunk_bytes=chunk_bytes, use_crc=use_crc, ecc=ecc, nsym=nsym, lm=provider)
    if not quality_gate:
        texts = _render_covers(payloads, seed_texts=seeds, quality=q, **kw)
        if return_attempts:
            return [(t, Attempt(s, {}, "base")) for t, s in zip(texts, seeds)]
        return texts
    thresholds = prepare_gate_thresholds(gate_thresholds)
    guard = _ensure_guard(quality_guard)
    total = max(regen_attempts, 0) + 1
    out: List[Any] = [None] * n
    last: Dict[int, tuple] = {}
    pending = list(range(n))
    # one schedule per distinct seed: the seeds differ per message, the overrides and variants per attempt do not
    schedules = {s: list(iter_attempts(s, regen_attempts, regen_strategy or {})) for s in set(seeds)}
    common = list(iter_attempts("", regen_attempts, regen_strategy or {}))
    for idx, att in enumerate(common, start=1):
        if not pending:
            break
        aq = dict(q)
        aq.update(att.overrides)
        atts = [schedules[seeds[i]][idx - 1] for i in pending]
        texts = _render_covers([payloads[i] for i in pending], seed_texts=[a.seed_text for a in atts], quality=aq,
                               **kw)
        verdicts: List[GuardResult] = guard.evaluate_batch(texts, thresholds)
        rejected = []
        for i, text, v, a in zip(pending, texts, verdicts, atts):
            status = "PASS" if v.passed else "REJECT"
            log.info("quality attempt %d/%d (%s) message %d -> %s %s", idx, total, att.seed_variant, i, status,
                     "; ".join(v.reasons))
            if v.passed:
                out[i] = (text, a) if return_attempts else text
            else:
                last[i] = (text, v)
                rejected.append(i)
        pending = rejected
    for i in pending:
        text, v = last[i]
        err = QualityGateError(text, list(v.reasons), dict(v.metrics))
        if not return_errors:
            raise err
        out[i] = err
    return out


def cover_generate(secret, *, seed_text: str, quality: Optional[Mapping[str, object]] = None, chunk_bytes: int = 256,
                   use_crc: bool = True, ecc: str = "rs", nsym: int = 10, lm=None, quality_gate: bool = True,
                   gate_thresholds: Optional[Mapping[str, float]] = None, regen_attempts: int = 2,
                   regen_strategy: Optional[Mapping[str, Any]] = None,
                   quality_guard: Optional[QualityGuard] = None) -> str:
    """``api.py:565-662``: one secret."""
    return cover_generate_batch([secret], seed_text=seed_text, quality=quality, chunk_bytes=chunk_bytes,
                                use_crc=use_crc, ecc=ecc, nsym=nsym, lm=lm, quality_gate=quality_gate,
                                gate_thresholds=gate_thresholds, regen_attempts=regen_attempts,
                                regen_strategy=regen_strategy, quality_guard=quality_guard)[0]


def _parse_spans_payload(payload: str) -> List[List[int]]:
    """``api.py:426-448``: a JSON list of int lists (or ``{"spans": [...]}``)."""
    try:
        obj = json.loads(payload)
    except json.JSONDecodeError as exc:
        raise ConfigurationError("cover text parsing not implemented; provide spans JSON input") from exc
    if isinstance(obj, Mapping):
        obj = obj.get("spans")
    if not isinstance(obj, Sequence):
        raise ConfigurationError("spans payload must be a sequence")
    spans = []
    for entry in obj:
        if not isinstance(entry, Sequence):
            raise ConfigurationError("span entry must be a sequence of integers")
        spans.append([int(v) for v in entry])
    return spans


def _span_end(bits, counts, toks, finish, sent_end) -> Optional[int]:
    """Index of the last token of the span that starts at ``toks[0]``, from the decoder's output for the
    remaining tokens: the packet (``bits`` read up to the JSON's closing brace) is complete after the first
    token whose cumulative bit count covers it (t*); with ``finish_sent`` the encoder then emitted top-1 tokens
    up to and including the first sentence-ending one AFTER t* (``code_base/arithmetic.py:114,134-137``: the
    test runs only on tail tokens).  None while the decoded prefix does not yet settle it."""
    from .exceptions import PacketECCError
    from .stego import bits_to_bytes_lsb, packet_prefix

    try:
        need = 8 * len(packet_prefix(bits_to_bytes_lsb(bits)))
    except PacketECCError:
        return None
    tstar = next((t for t, c in enumerate(counts) if c >= need), None)
    if tstar is None:
        return None
    if not finish:
        return tstar
    for t in range(tstar + 1, len(counts)):
        if sent_end[int(toks[t])]:
            return t
    if len(counts) == len(toks):  # the text ends inside the tail (stripped / truncated cover)
        return len(toks) - 1
    return None


def _split_double_newlines(ids: List[int], tok) -> List[int]:
    """``code_base/arithmetic.py:233-242``: a re-tokenised "\\n\\n" (GPT-2 id 628, which the coder never emits:
    it is banned) is split back into two "\\n" (id 198) -- applied when the tokenizer has those pieces."""
    if 628 not in ids:
        return ids
    try:
        if tok.decode([628]) != "\n\n" or tok.decode([198]) != "\n":
            return ids
    except Exception:  # noqa: BLE001 - a vocabulary without those ids
        return ids
    out: List[int] = []
    for t in ids:
        out.extend((198, 198) if t == 628 else (t,))
    return out


def _cover_ids(text: str, seed_text: str, seed_ids: List[int], tok) -> Optional[List[int]]:
    """The cover's token ids after the seed: the text's ids minus the seed's, or -- when the seed's last token
    merged with the first cover token on re-tokenisation -- the ids of the text after the decoded seed."""
    ids = seed_to_ids(text, tok)
    if ids[: len(seed_ids)] == seed_ids:
        return ids[len(seed_ids):]
    seed_str = spans_to_text([], seed_ids, tok)
    if seed_str and text.startswith(seed_str):
        return seed_to_ids(text[len(seed_str):], tok) if text[len(seed_str):] else []
    return None


def _quality_key(q: Mapping[str, Any]) -> str:
    return repr(sorted(((str(k), v) for k, v in q.items())))


def _text_qualities(quality, qualities, n: int) -> Optional[List[Dict[str, Any]]]:
    """One merged quality per text for ``qualities`` (None without them); at most one of the two is given."""
    if qualities is None:
        return None
    if quality is not None:
        raise ConfigurationError("give exactly one of quality (shared) and qualities (one per text)")
    qs = [normalise_quality(q) for q in qualities]
    if len(qs) != n:
        raise ConfigurationError(f"{len(qs)} qualities for {n} texts")
    return qs


def _cover_rests(texts: Sequence[str], seeds: Sequence[str], tok) -> List[List[int]]:
    """Every cover's token ids after its own seed (``_cover_ids``, double newlines split back)."""
    from .codec.errors import DecodeDivergenceError

    seed_ids = {s: seed_to_ids(s, tok) for s in set(seeds)}
    rest: List[List[int]] = []
    for i, text in enumerate(texts):
        ids = _cover_ids(text, seeds[i], seed_ids[seeds[i]], tok)
        if ids is None:
            raise DecodeDivergenceError(f"cover {i} does not start with the seed text")
        rest.append(_split_double_newlines(ids, tok))
    return rest


def _spans_by_rounds(rest: List[List[int]], seeds: Sequence[Any], contexts: Mapping[Any, List[int]], lm,
                     quality: Optional[Mapping[str, object]], labels=None) -> List[List[List[int]]]:
    """The round-based span search of :func:`texts_to_spans` over the covers' ids after their seeds (``rest``; the
    lists are replaced as spans are found): text i is decoded after ``contexts[seeds[i]]`` with the one ``quality``.
    ``labels``: the texts' numbers in the caller's call, for the error messages."""
    from .codec.errors import DecodeDivergenceError
    from .lm.mock import MockLM
    from .stego import _quality_args, _takes_contexts

    rest = list(rest)
    q = _quality_args(quality)
    finish = bool(q.get("finish_sent")) and hasattr(lm, "sentence_end_table")
    sent_end = lm.sentence_end_table() if finish else None
    if hasattr(lm, "decode_counted_repair"):
        entry = lm.decode_counted_repair
    elif hasattr(lm, "decode_counted"):
        entry = lm.decode_counted
    elif isinstance(lm, MockLM):
        entry = None
    else:
        raise NotImplementedError("text_to_spans needs a provider with decode_counted (or the mock)")

    def decode_round(members: List[int], context=None, per_stream=None):
        """One lockstep decode of the next span of ``members``, after the shared ``context`` or one context per
        stream: (bits, counts, lists, edits, originals)."""
        lists = [rest[i] for i in members]
        args, ckw = ((context,), {}) if per_stream is None else ((), {"contexts": per_stream})

        def settled(bits_l, counts_l, toks_l=None):
            toks_l = lists if toks_l is None else toks_l
            return all(_span_end(b, c, l, finish, sent_end) is not None for b, c, l in zip(bits_l, counts_l, toks_l))

        edits_l = [[] for _ in lists]
        orig = [list(l) for l in lists]
        if entry is None:  # the mock's identity coder: 8 bits per token
            bits_l = [lm.decode_arithmetic(l, context, quality=q) for l in lists]
            counts_l = [[8 * (t + 1) for t in range(len(l))] for l in lists]
        elif hasattr(lm, "decode_counted_repair"):
            bits_l, counts_l, lists, edits_l = entry(lists, *args, quality=q, done=settled, **ckw)
        else:
            bits_l, counts_l = entry(lists, *args, quality=q, done=settled, **ckw)
        return bits_l, counts_l, lists, edits_l, orig

    spans: List[List[List[int]]] = [[] for _ in rest]
    active = [i for i in range(len(rest)) if rest[i]]
    while active:
        distinct = list(dict.fromkeys(seeds[i] for i in active))
        if len(distinct) == 1:
            runs = [(active, {"context": contexts[distinct[0]]})]
        elif entry is not None and _takes_contexts(entry):
            runs = [(active, {"per_stream": [contexts[seeds[i]] for i in active]})]
        else:  # one lockstep batch per distinct context
            runs = [([i for i in active if seeds[i] == s], {"context": contexts[s]}) for s in distinct]
        ends: Dict[int, tuple] = {}
        for members, ckw in runs:
            for i, b, c, l, ed, o in zip(members, *decode_round(members, **ckw)):
                ends[i] = (b, c, l, ed, o)
        nxt = []
        for i in active:
            b, c, l, ed, o = ends[i]
            end = _span_end(b, c, l, finish, sent_end)
            if end is None:
                raise DecodeDivergenceError(f"cover {labels[i] if labels is not None else i}: no complete packet in "
                                            f"the remaining {len(l)} tokens")
            # the list as it stood after the last repair inside the span (later "repairs" decoded the next span's
            # tokens out of context); a repair at the span's end may have split a cross-boundary merge, whose
            # suffix tokens start the next span
            l = next((snap for p, snap in reversed(ed) if p <= end), o)
            spans[i].append([int(t) for t in l[: end + 1]])
            rest[i] = l[end + 1:]
            if rest[i]:
                nxt.append(i)
        active = nxt
    return spans


def texts_to_spans(texts: Sequence[str], *, seed_text: Optional[str] = None,
                   seed_texts: Optional[Sequence[str]] = None, lm,
                   quality: Optional[Mapping[str, object]] = None,
                   qualities: Optional[Sequence[Optional[Mapping[str, object]]]] = None,
                   slots: Optional[int] = None) -> List[List[List[int]]]:
    """Recover the token spans of many cover texts (the inverse of ``spans_to_text``, which the reference leaves
    unimplemented, ``codec/textio.py:58-63``).  The text is re-tokenised, the seed's ids are stripped, and the
    spans are found one per round: every cover's next span is decoded as one stream of a lockstep batch, the
    packet completes at a known token and the span ends there or, with ``finish_sent``, at the following
    sentence end.  A text that re-tokenises differently from the emitted ids (GPT-2 BPE merges, also across
    span boundaries) is repaired while decoding with the reference's heuristics (``code_base/arithmetic.py:
    233-242,300-342``, the provider's ``decode_counted_repair``): the spans are the repaired ids.

    Exactly one of ``seed_text`` (shared) and ``seed_texts`` (one per text) is given.  With ``seed_texts`` every
    text is stripped of its own seed and decoded after its own context: one lockstep batch with one context per
    stream on a provider whose counted decodes take ``contexts=``, one batch per distinct context otherwise.

    ``qualities`` (one mapping per text, instead of ``quality``): every text is decoded with its own quality -- the
    covers of one ``cover_generate_batch`` call were accepted at different attempts, each with that attempt's
    overrides.  With ``qualities`` or ``slots`` a provider that has ``reveal_spans`` (the HIP provider) finds the
    spans of all texts in one slot-scheduled batch through ``slots`` slots; any other provider is called as without
    them, once per distinct quality, results in the caller's order.  Without both the call is the round-based one
    described above."""
    tok = _tokenizer_of(lm)
    seed_text, seeds = _one_or_many_seeds(seed_text, seed_texts, len(texts))
    if seeds is None:
        seeds = [seed_text] * len(texts)
    per_q = _text_qualities(quality, qualities, len(texts))
    if slots is not None and int(slots) < 1:
        raise ConfigurationError("slots must be positive")
    contexts = {s: list(lm.encode_seed(s)) for s in set(seeds)}
    rest = _cover_rests(texts, seeds, tok)
    if per_q is None and slots is None:
        return _spans_by_rounds(rest, seeds, contexts, lm, quality)
    from .stego import _quality_args

    merged = [_quality_args(q) for q in per_q] if per_q is not None else [_quality_args(quality)] * len(texts)
    if hasattr(lm, "reveal_spans"):
        return lm.reveal_spans(rest, contexts=[contexts[s] for s in seeds], qualities=merged, slots=slots)
    groups: Dict[str, List[int]] = {}
    for i, q in enumerate(merged):
        groups.setdefault(_quality_key(q), []).append(i)
    out: List[Any] = [None] * len(texts)
    for members in groups.values():
        got = _spans_by_rounds([rest[i] for i in members], [seeds[i] for i in members], contexts, lm,
                               merged[members[0]], labels=members)
        for i, sp in zip(members, got):
            out[i] = sp
    return out


def _looks_like_spans_json(text: str) -> bool:
    try:
        _parse_spans_payload(text)
        return True
    except ConfigurationError:
        return False


def cover_reveal_batch(cover_texts: Sequence[str], *, seed_text: Optional[str] = None,
                       seed_texts: Optional[Sequence[str]] = None, quality: Optional[Mapping[str, object]] = None,
                       use_crc: bool = True, ecc: str = "rs", nsym: int = 10, lm=None,
                       return_errors: bool = False,
                       qualities: Optional[Sequence[Optional[Mapping[str, object]]]] = None,
                       attempts: Optional[Sequence[Attempt]] = None, slots: Optional[int] = None) -> List[Any]:
    """:func:`cover_reveal` for many covers: spans of all texts recovered round by round in lockstep batches,
    then one batched ``stego_decode``.  Exactly one of ``seed_text`` (shared) and ``seed_texts`` (one per cover: the
    seed of the attempt that produced it, ``cover_generate_batch(..., return_attempts=True)``) is given.

    ``qualities`` (one mapping per cover, instead of ``quality``) reveals every cover with its own quality;
    ``attempts`` -- the :class:`Attempt` objects ``cover_generate_batch(return_attempts=True)`` returned with the
    covers -- is shorthand for ``seed_texts=[a.seed_text ...]`` and ``qualities=[{**quality, **a.overrides} ...]``, so
    the output of one ``cover_generate_batch`` call is revealed in one call whatever attempt accepted each cover
    (``attempts`` with ``seed_text``, ``seed_texts`` or ``qualities``: ``ConfigurationError``).  With ``qualities``,
    ``attempts`` or ``slots`` the spans are found by :func:`texts_to_spans` with them (one slot-scheduled batch on the
    HIP provider), and every packet of a cover is decoded with its cover's quality."""
    from .stego import stego_decode_batch

    n = len(cover_texts)
    if attempts is not None:
        if seed_text is not None or seed_texts is not None or qualities is not None:
            raise ConfigurationError("attempts already gives every cover's seed and quality: give neither "
                                     "seed_text / seed_texts nor qualities with it")
        attempts = list(attempts)
        if len(attempts) != n:
            raise ConfigurationError(f"{len(attempts)} attempts for {n} covers")
        base = normalise_quality(quality)
        seed_texts = [a.seed_text for a in attempts]
        qualities = [{**base, **normalise_quality(a.overrides)} for a in attempts]
        quality = None
    seed_text, seeds = _one_or_many_seeds(seed_text, seed_texts, n)
    provider = _ensure_cover_lm(lm)
    per_q = _text_qualities(quality, qualities, n)
    q = normalise_quality(quality)
    qkw = {"quality": q} if per_q is None else {"qualities": per_q}
    span_sets: List[Any] = [None] * n
    plain = []
    for i, text in enumerate(cover_texts):
        if _looks_like_spans_json(text):
            span_sets[i] = _parse_spans_payload(text)
        else:
            plain.append(i)
    if plain:
        skw = {"seed_text": seed_text} if seeds is None else {"seed_texts": [seeds[i] for i in plain]}
        tkw = {"quality": q} if per_q is None else {"qualities": [per_q[i] for i in plain]}
        if slots is not None:
            tkw["slots"] = slots
        for i, sp in zip(plain, texts_to_spans([cover_texts[i] for i in plain], lm=provider, **tkw, **skw)):
            span_sets[i] = sp
    skw = {"seed_text": seed_text} if seeds is None else {"seed_texts": seeds}
    return stego_decode_batch(span_sets, use_crc=use_crc, ecc=ecc, nsym=nsym, lm=provider,
                              return_errors=return_errors, **qkw, **skw)


def cover_reveal(cover_text: str, *, seed_text: str, quality: Optional[Mapping[str, object]] = None,
                 use_crc: bool = True, ecc: str = "rs", nsym: int = 10, lm=None,
                 slots: Optional[int] = None) -> bytes:
    """``api.py:665-704``: a JSON spans payload is decoded as in the reference; a cover TEXT has its spans
    recovered by :func:`texts_to_spans` (the reference's ``text_to_spans`` raises ``NotImplementedError``,
    after which it can only parse JSON), then ``stego_decode``.  ``slots`` is passed on to :func:`texts_to_spans`."""
    provider = _ensure_cover_lm(lm)
    q = normalise_quality(quality)
    if _looks_like_spans_json(cover_text):
        spans = _parse_spans_payload(cover_text)
    else:
        tok = getattr(provider, "tokenizer", None)
        try:
            if tok is None:
                raise NotImplementedError
            skw = {} if slots is None else {"slots": slots}
            spans = text_to_spans(cover_text, seed_to_ids(seed_text, tok), tok, lm=provider, quality=q,
                                  seed_text=seed_text, **skw)
        except NotImplementedError:
            spans = _parse_spans_payload(cover_text)
    return stego_decode(spans, use_crc=use_crc, ecc=ecc, nsym=nsym, quality=q, seed_text=seed_text, lm=provider)


__all__ = ["cover_generate", "cover_generate_batch", "cover_reveal", "cover_reveal_batch", "texts_to_spans",
           "iter_attempts", "prepare_gate_thresholds",
           "prepare_regen_strategy", "DEFAULT_GATE_THRESHOLDS", "DEFAULT_REGEN_STRATEGY", "Attempt"]
