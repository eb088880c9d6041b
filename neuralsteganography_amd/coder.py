"""Batched arithmetic-coding sessions on the HIP coder (``libnsgcoder.so``).

A session owns the device buffers of B independent streams and launches one coder step per call on the
current torch stream.  It is the batched replacement of the per-stream loops in
``code_base/arithmetic.py:112-210`` (encode) and ``:254-371`` (decode): the caller supplies the ``[B, ld]``
logits of each step (a GPT-2 forward, or synthetic rows) and the kernel does sort/softmax/CDF/interval
work for all B streams at once.

All device state lives in torch tensors (PyTorch is plumbing here); the arithmetic runs only in the HIP
kernel.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .codec.errors import ArithmeticRangeError, DecodeDivergenceError
from .exceptions import ConfigurationError


def _torch():
    import torch

    return torch


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream_handle():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def row_stride(vocab: int, dtype: str) -> int:
    """Padded logits row stride the kernel wants: a multiple of 64 elements (16-byte vectors, 256-B rows)."""
    _ = dtype
    return ((vocab + 63) // 64) * 64


@dataclass(frozen=True)
class CoderParams:
    """Coder parameters of ``encode_arithmetic``/``decode_arithmetic`` (``code_base/arithmetic.py:78-88``)."""

    vocab: int
    precision: int = 26
    temp: float = 0.9
    topk: int = 300
    dtype: str = "f32"  # logits dtype: "f32" or "f16"; "f64": a provider's probability rows (rank coder only)
    banned: Optional[Sequence[int]] = None  # default: (vocab-1, 628) as arithmetic.py:124-125

    def banned_ids(self) -> List[int]:
        if self.banned is not None:
            return [int(b) for b in self.banned]
        return [self.vocab - 1, 628]

    @property
    def dtype_code(self) -> int:
        if self.dtype == "f32":
            return _lib.NS_DTYPE_F32
        if self.dtype == "f16":
            return _lib.NS_DTYPE_F16
        if self.dtype == "f64":
            return _lib.NS_DTYPE_F64
        raise ConfigurationError(f"unsupported logits dtype {self.dtype!r}")

    @property
    def torch_dtype(self):
        torch = _torch()
        return {"f16": torch.float16, "f64": torch.float64}.get(self.dtype, torch.float32)

    def validate(self) -> None:
        if self.vocab < 2:
            raise ConfigurationError("vocab must be >= 2")
        if not 1 <= self.precision <= 60:
            raise ConfigurationError("precision must be within [1, 60]")
        if not self.temp > 0:
            raise ConfigurationError("temperature must be positive")
        if self.topk < 1:
            raise ConfigurationError("topk must be positive")
        if len(self.banned_ids()) > _lib.NS_MAX_BANNED:
            raise ConfigurationError(f"at most {_lib.NS_MAX_BANNED} banned ids")


class StreamQuality:
    """Per-stream coder quality rows (``ns_stream_quality``) for one call: row i is what the step kernel derives
    from ``params[i]`` (temp, topk, precision), filled by ``ns_stream_quality_fill`` -- the derived values, the
    speculative-sample rule included, live in the library only.  ``k_max`` (default: the largest topk) is the
    value every launch decision of the call follows; all rows share vocab, dtype and banned ids."""

    def __init__(self, params: Sequence[CoderParams], k_max: Optional[int] = None):
        params = list(params)
        if not params:
            raise ConfigurationError("StreamQuality needs at least one stream")
        head = params[0]
        for q in params:
            q.validate()
            if (q.vocab, q.dtype, q.banned_ids()) != (head.vocab, head.dtype, head.banned_ids()):
                raise ConfigurationError("the streams of one call share vocab, logits dtype and banned ids")
        self.params = params
        self.k_max = int(k_max) if k_max is not None else max(q.topk for q in params)
        ban = head.banned_ids()
        cban = (ctypes.c_int32 * max(1, len(ban)))(*ban)
        rows = (_lib.NsStreamQuality * len(params))()
        L = _lib.lib()
        for i, q in enumerate(params):
            rc = L.ns_stream_quality_fill(q.vocab, cban, len(ban), float(q.temp), int(q.topk), int(q.precision),
                                          self.k_max, ctypes.byref(rows[i]))
            if rc != _lib.NS_OK:
                raise ConfigurationError(f"stream {i}: {L.ns_last_error(None).decode()}")
        # [n, 4] int64: the 32-byte rows as the device table holds them (indexable like the state rows)
        self.rows = np.frombuffer(bytes(rows), dtype=np.int64).reshape(len(params), 4).copy()
        self.precisions = np.asarray([q.precision for q in params], dtype=np.int64)

    def __len__(self) -> int:
        return len(self.params)

    @property
    def max_precision(self) -> int:
        return int(self.precisions.max())

    def take(self, idx: Sequence[int]) -> "StreamQuality":
        """The rows of streams ``idx`` (same ``k_max``: rows are only valid for the call they were filled for)."""
        idx = np.asarray(idx, dtype=np.int64)
        out = StreamQuality.__new__(StreamQuality)
        out.params = [self.params[int(i)] for i in idx]
        out.k_max = self.k_max
        out.rows, out.precisions = self.rows[idx].copy(), self.precisions[idx].copy()
        return out

    def context_params(self) -> CoderParams:
        """Parameters of the coder context that serves the call: topk ``k_max`` and the largest precision (with a
        table registered the kernel reads neither, nor the temperature, from the context)."""
        head = self.params[0]
        return CoderParams(vocab=head.vocab, precision=self.max_precision, temp=1.0, topk=self.k_max, dtype=head.dtype,
                           banned=head.banned)

    def table(self, device):
        torch = _torch()
        return torch.from_numpy(self.rows).to(device)

    def init_rows(self, device):
        """[n, 4] int64 fresh coder states, ``hi = 2^precision`` of each row."""
        torch = _torch()
        st = np.zeros((len(self.precisions), 4), dtype=np.int64)
        st[:, 1] = np.left_shift(np.int64(1), self.precisions)
        return torch.from_numpy(st).to(device)


def _check_quality(ctx: "CoderContext", B: int, quality: Optional[StreamQuality]) -> None:
    if quality is None:
        return
    if len(quality) != B:
        raise ConfigurationError(f"{len(quality)} quality rows for {B} streams")
    if quality.k_max > ctx.params.topk:
        raise ConfigurationError("the coder context's topk must cover the quality table's k_max")


class _table_registered:
    """``ns_set_stream_quality`` around a call (None: nothing to do), cleared on exit like ``ns_set_stats``; a
    ``k_max`` beyond the single-pass limit goes through ``ns_set_stream_quality_wide`` (the wide kernels read the
    rows)."""

    def __init__(self, ctx: "CoderContext", table, k_max: int):
        self.ctx, self.table, self.k_max = ctx, table, k_max

    def __enter__(self):
        if self.table is not None:
            L = _lib.lib()
            entry = L.ns_set_stream_quality_wide if int(self.k_max) > self.ctx.single_pass_limit \
                else L.ns_set_stream_quality
            self.ctx.check(entry(self.ctx._h, _ptr(self.table), int(self.k_max)), "ns_set_stream_quality")

    def __exit__(self, *exc):
        if self.table is not None and self.ctx._h:
            _lib.lib().ns_set_stream_quality(self.ctx._h, ctypes.c_void_p(0), 0)
        return False


_DEFERRED: List[tuple] = []  # (device, handle) of contexts closed during a graph capture


def _destroy(device: int, h) -> None:
    torch = _torch()
    if torch.cuda.is_available():  # launches still queued may read the context's buffers
        torch.cuda.synchronize(device)
    _lib.lib().ns_destroy(h)


def _drain_deferred() -> None:
    torch = _torch()
    if not _DEFERRED or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        return
    while _DEFERRED:
        dev, h = _DEFERRED.pop()
        _destroy(dev, h)


class CoderContext:
    """Owns an ``ns_ctx`` (device, vocab, precision, dtype, max batch)."""

    def __init__(self, params: CoderParams, max_batch: int, device: Optional[int] = None):
        params.validate()
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.NativeLibraryError("the HIP coder needs a ROCm GPU (torch.cuda.is_available() is False)")
        _drain_deferred()
        self.params = params
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.max_batch = int(max_batch)
        L = _lib.lib()
        vocab_valid = params.vocab - len({b for b in params.banned_ids() if 0 <= b < params.vocab})
        self.K = min(params.topk, vocab_valid)
        self.single_pass_limit = int(L.ns_max_topk(params.dtype_code))
        self.wide = self.K > self.single_pass_limit  # large top-k: multi-kernel wide path
        handle = L.ns_create(self.device, self.max_batch, params.vocab, max(1, self.K), params.precision,
                             params.dtype_code)
        if not handle:
            raise _lib.NativeLibraryError(f"ns_create failed: {L.ns_last_error(None).decode()}")
        self._h = ctypes.c_void_p(handle)
        self._banned = (ctypes.c_int32 * max(1, len(params.banned_ids())))(*params.banned_ids())
        self._nbanned = len(params.banned_ids())

    def check(self, rc: int, what: str) -> None:
        if rc != _lib.NS_OK:
            msg = _lib.lib().ns_last_error(self._h).decode()
            if rc == _lib.NS_ERR_CONFIG:
                raise ConfigurationError(f"{what}: {msg}")
            raise _lib.NativeLibraryError(f"{what}: rc={rc}: {msg}")

    def set_sentence_end(self, table) -> None:
        """Register a device uint8 table [vocab] (nonzero = sentence-ending token) for finish_sent."""
        torch = _torch()
        if table is None:
            self._sent_end = None
            self.check(_lib.lib().ns_set_sentence_end(self._h, ctypes.c_void_p(0)), "ns_set_sentence_end")
            return
        t = torch.as_tensor(table, dtype=torch.uint8).to(torch.device("cuda", self.device)).contiguous()
        if t.numel() != self.params.vocab:
            raise ConfigurationError("sentence-end table must have one entry per vocabulary id")
        self._sent_end = t  # keep alive: the library holds the raw pointer
        self.check(_lib.lib().ns_set_sentence_end(self._h, _ptr(t)), "ns_set_sentence_end")

    def counters(self) -> List[int]:
        out = (ctypes.c_uint64 * 4)()
        self.check(_lib.lib().ns_read_counters(self._h, out), "ns_read_counters")
        return [int(v) for v in out]

    def close(self) -> None:
        """Release the context.  Launches still queued may read its buffers, so the device is synchronised
        first -- except while the current stream is capturing a hipGraph (a garbage-collected context during
        a capture): a device-wide sync or a free there would invalidate the capture, so the handle is parked
        and destroyed by the next close() or context creation outside a capture."""
        h = getattr(self, "_h", None)
        if not h:
            return
        self._h = None
        torch = _torch()
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            _DEFERRED.append((self.device, h))
            return
        _destroy(self.device, h)
        _drain_deferred()

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


def _check_logits(ctx: "CoderContext", B: int, logits) -> None:
    """Host-side validation before any launch that reads a logit matrix: dtype of the context, [B, ld] with
    unit column stride, ld >= vocab, on this context's device (a mismatch would make the kernel misread rows
    or read past their end)."""
    p = ctx.params
    if logits.dtype != p.torch_dtype or logits.dim() != 2 or logits.shape[0] != B:
        raise ConfigurationError(f"logits must be [{B}, ld] {p.dtype}")
    if logits.stride(1) != 1 or logits.shape[1] < p.vocab or logits.stride(0) < p.vocab or not logits.is_cuda:
        raise ConfigurationError("logits must be contiguous rows on the GPU with ld >= vocab")
    if logits.device.index != ctx.device:
        raise ConfigurationError(f"logits on cuda:{logits.device.index}, coder context on cuda:{ctx.device}")


def _rank_rows(ctx: "CoderContext", B: int, rows, q):
    """The device matrix a rank step reads: logits as they are (checked), or a provider step's
    :class:`~neuralsteganography_amd.codec.distribution.ProbRows` registered with ``ns_set_rank_rows`` (the
    reference's quality errors raised on the host first)."""
    if not getattr(rows, "prob_rows", False):
        if ctx.params.dtype == "f64":
            # an f64 context reads rk_count / rk_idmap registered for ProbRows: a plain matrix would leave it reading
            # an earlier step's (possibly freed) tensors
            raise ConfigurationError("a coder context of dtype 'f64' takes provider ProbRows only")
        _check_logits(ctx, B, rows)
        return rows
    if ctx.params.dtype != "f64":
        raise ConfigurationError("provider probability rows need a coder context of dtype 'f64'")
    if rows.ncols > ctx.params.vocab:
        raise ConfigurationError(f"a row of {rows.ncols} entries exceeds the context's {ctx.params.vocab}")
    rows.check_quality(q)
    _check_logits(ctx, B, rows.values)
    idm = rows.idmap
    ctx.check(_lib.lib().ns_set_rank_rows(ctx._h, _ptr(rows.count), _ptr(idm), idm.stride(0) if idm is not None else 0,
                                          int(rows.dict_rows)), "ns_set_rank_rows")
    return rows.values


def _state_tensor(B: int, device):
    torch = _torch()
    return torch.zeros((B, 4), dtype=torch.int64, device=device)


def _state_fields(state) -> dict:
    """Host view of [B,4] int64 state rows: lo, hi, bit_pos, ntokens, flags."""
    s = state.cpu().numpy()
    w32 = s.view(np.int32).reshape(s.shape[0], 8)
    return {"lo": s[:, 0].view(np.uint64), "hi": s[:, 1].view(np.uint64), "bit_pos": s[:, 2],
            "ntokens": w32[:, 6], "flags": w32[:, 7].view(np.uint32)}


def _stats_rows(acc: np.ndarray, bits_consumed: Optional[np.ndarray] = None) -> List[dict]:
    """[B, 4] accumulators (sum log p, sum KL bits, sum H bits, n) -> the reference's averages per stream
    (``code_base/arithmetic.py:212-215``, ``sample.py:50-52``); NaN where a stream had no counted step."""
    out = []
    for i in range(acc.shape[0]):
        n = acc[i, 3]
        d = {"avg_NLL": -acc[i, 0] / n if n else math.nan, "avg_KL": acc[i, 1] / n if n else math.nan,
             "avg_Hq": acc[i, 2] / n if n else math.nan}
        if bits_consumed is not None:
            d["words_per_bit"] = n / bits_consumed[i] if bits_consumed[i] else math.nan
        out.append(d)
    return out


def _bit_array(bits) -> np.ndarray:
    """A payload bit list as uint8 (nonzero = 1 after packing).  Python lists go through ``bytes`` (one C pass,
    ≈3x faster than numpy's per-object conversion: 4,096 KiB-payload lists are ≈1 s of host time otherwise)."""
    if isinstance(bits, (list, tuple)):
        try:
            return np.frombuffer(bytes(bits), dtype=np.uint8)
        except (ValueError, TypeError):
            pass
    return np.asarray(bits, dtype=np.uint8)


def _rows_to_lists(dev_rows, lengths) -> List[List[int]]:
    """Row i's first lengths[i] entries of a device [B, cap] int array as Python int lists: only the columns in
    use cross PCIe (the history buffer is sized for the KV budget, far wider than a finished job's tokens), and
    the rows become lists in one conversion."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.max(initial=0))
    if n == 0:
        return [[] for _ in range(dev_rows.shape[0])]
    rows = dev_rows[:, :n].cpu().numpy().tolist()
    return [r[:k] if k < n else r for r, k in zip(rows, lengths.tolist())]


def _bit_rows_to_lists(dev_bytes, nbits) -> List[List[int]]:
    """Row i's first nbits[i] bits (LSB-first bytes on the device) as Python int lists."""
    nbits = np.asarray(nbits, dtype=np.int64)
    nb = int(nbits.max(initial=0))
    if nb == 0:
        return [[] for _ in range(dev_bytes.shape[0])]
    host = dev_bytes[:, : (nb + 7) // 8].cpu().numpy()
    rows = np.unpackbits(host, axis=1, bitorder="little")[:, :nb].tolist()
    return [r[:k] if k < nb else r for r, k in zip(rows, nbits.tolist())]


class EncodeSession:
    """B streams being encoded; call :meth:`step` once per generated token with that step's logits.

    ``stats=True`` also accumulates the statistics ``encode_arithmetic`` returns (avg_NLL, avg_KL,
    words_per_bit, avg_Hq; ``code_base/arithmetic.py:193-217``) on the device -- within a float64
    tolerance of the reference, not bit-exact -- at the cost of a heavier kernel build."""

    def __init__(self, ctx: CoderContext, payload_bits: Sequence[Sequence[int]], max_tokens: Optional[int] = None,
                 stats: bool = False, payload_stride: Optional[int] = None,
                 quality: Optional[StreamQuality] = None):
        torch = _torch()
        self.ctx = ctx
        self.B = len(payload_bits)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        _check_quality(ctx, self.B, quality)
        dev = torch.device("cuda", ctx.device)
        # per-stream quality rows (None: the context's one quality for every stream), [B, 4] int64 = 32-byte rows
        self.qtable = quality.table(dev) if quality is not None else None
        self.k_max = quality.k_max if quality is not None else 0
        self.nbits_host = np.asarray([len(b) for b in payload_bits], dtype=np.int64)
        stride = max(1, int((self.nbits_host.max() + 7) // 8), int(payload_stride or 0))
        pl = np.zeros((self.B, stride), dtype=np.uint8)
        for i, bits in enumerate(payload_bits):
            if len(bits):
                packed = np.packbits(_bit_array(bits), bitorder="little")
                pl[i, : packed.size] = packed
        self.payload = torch.from_numpy(pl).to(dev)
        self.nbits = torch.from_numpy(self.nbits_host).to(dev)
        self.state = _state_tensor(self.B, dev)
        with _table_registered(ctx, self.qtable, self.k_max):
            ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        cap = max_tokens if max_tokens is not None else int(2 * self.nbits_host.max() + 64)
        self.hist = torch.full((self.B, cap), -1, dtype=torch.int32, device=dev)
        self.trace = None
        self.steps = 0
        self.stats_acc = torch.zeros((self.B, 4), dtype=torch.float64, device=dev) if stats else None

    def enable_trace(self):
        torch = _torch()
        self.trace = torch.zeros((self.B, 4), dtype=torch.int64, device=self.state.device)
        return self.trace

    def stats(self) -> List[dict]:
        """Per-stream avg_NLL, avg_KL, words_per_bit, avg_Hq (as ``encode_arithmetic`` returns them)."""
        if self.stats_acc is None:
            raise ConfigurationError("the session was created without stats=True")
        return _stats_rows(self.stats_acc.cpu().numpy(), self.fields()["bit_pos"])

    def step(self, logits, *, force_exact: bool = False, finish_sent: bool = False, diag_flags: int = 0):
        """One coder step on ``logits`` ([B, ld] contiguous rows, ld = :func:`row_stride`).

        ``finish_sent``: once a stream's payload is consumed it keeps emitting top-1 tokens until a
        sentence-ending one (needs :meth:`CoderContext.set_sentence_end`).  ``diag_flags``
        (NS_STEP_DIAG_*) are for phase timing only: such a step advances no state."""
        p = self.ctx.params
        self._check_logits(logits)
        flags = (_lib.NS_STEP_FORCE_EXACT_SUM if force_exact else 0) | int(diag_flags)
        if finish_sent:
            flags |= _lib.NS_STEP_FINISH_SENT
        L = _lib.lib()
        if self.stats_acc is not None:
            self.ctx.check(L.ns_set_stats(self.ctx._h, _ptr(self.stats_acc)), "ns_set_stats")
        with _table_registered(self.ctx, self.qtable, self.k_max):
            rc = L.ns_encode_step(
                self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.payload), self.payload.stride(0),
                _ptr(self.nbits), _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), self.hist.shape[1],
                float(p.temp), int(p.topk), self.ctx._banned, self.ctx._nbanned, _ptr(self.trace), flags,
                _stream_handle())
        if self.stats_acc is not None:
            L.ns_set_stats(self.ctx._h, ctypes.c_void_p(0))
        self.ctx.check(rc, "ns_encode_step")
        self.steps += 1
        return self.out_token

    def _check_logits(self, logits) -> None:
        _check_logits(self.ctx, self.B, logits)

    def all_done(self) -> bool:
        return bool(np.all(_state_fields(self.state)["flags"] & _lib.NS_ST_DONE))

    def mark_done(self, streams: Sequence[int]) -> None:
        """Stop ``streams`` (host decision, e.g. the reference's '<eos>' text check, arithmetic.py:208-210)."""
        torch = _torch()
        idx = torch.tensor(list(streams), device=self.state.device, dtype=torch.long)
        w = self.state.view(torch.int32)
        w[idx, 7] = w[idx, 7] | _lib.NS_ST_DONE

    def ensure_history(self, steps_ahead: int) -> None:
        """Grow the device token history so ``steps_ahead`` more steps fit (finish_sent tails are unbounded)."""
        need = int(self.fields()["ntokens"].max(initial=0)) + int(steps_ahead)
        cap = self.hist.shape[1]
        if need <= cap:
            return
        torch = _torch()
        new = torch.full((self.B, max(need, 2 * cap)), -1, dtype=torch.int32, device=self.hist.device)
        new[:, :cap] = self.hist
        self.hist = new

    def fields(self) -> dict:
        return _state_fields(self.state)

    # ---------------------------------------------------------------- slots (lm/slots.py: refill, compaction)
    def load_slots(self, slots: Sequence[int], payload_bits: Sequence[Sequence[int]],
                   quality: Optional[StreamQuality] = None) -> None:
        """Start new payloads in ``slots`` (rows of this session): payload row, bit count, a fresh coder state
        (``ns_init_state``'s values) and, with stats, zeroed accumulators.  The token history row is reused from
        position 0 (only the first ``ntokens`` entries of a row are ever read).  A session with per-stream quality
        takes the admitted streams' rows in ``quality`` (filled for the session's ``k_max``): the table rows are
        written with the payload, and each fresh state starts at its row's ``2^precision``."""
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        stride = self.payload.shape[1]
        pl = np.zeros((n, stride), dtype=np.uint8)
        nb = np.zeros(n, dtype=np.int64)
        for i, bits in enumerate(payload_bits):
            nb[i] = len(bits)
            if len(bits):
                packed = np.packbits(_bit_array(bits), bitorder="little")
                if packed.size > stride:
                    raise ConfigurationError("payload longer than the session's payload stride")
                pl[i, : packed.size] = packed
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.payload[idx] = torch.from_numpy(pl).to(dev)
        self.nbits[idx] = torch.from_numpy(nb).to(dev)
        self.nbits_host[np.asarray(slots)] = nb
        if (quality is None) != (self.qtable is None):
            raise ConfigurationError("load_slots: quality rows go with a session created with per-stream quality")
        if quality is not None:
            if len(quality) != n or quality.k_max != self.k_max:
                raise ConfigurationError("load_slots: one quality row per slot, filled for the session's k_max")
            self.qtable[idx] = quality.table(dev)
            self.state[idx] = quality.init_rows(dev)
        else:
            self.state[idx] = self.init_row().expand(n, 4)
        if self.stats_acc is not None:
            self.stats_acc[idx] = 0

    def init_row(self, precision: Optional[int] = None):
        """[1, 4] int64: the state ``ns_init_state`` writes (lo 0, hi 2^precision, bit_pos 0, ntokens | flags 0);
        ``precision``: that of the stream's quality row (default: the context's)."""
        torch = _torch()
        P = self.ctx.params.precision if precision is None else int(precision)
        return torch.tensor([[0, 1 << P, 0, 0]], dtype=torch.int64, device=self.state.device)

    def park_slots(self, slots: Sequence[int]) -> None:
        """Mark ``slots`` finished (NS_ST_DONE): the coder step and the decode attention skip them (empty slots;
        their quality rows stay as they are -- a finished stream's row is never read)."""
        if len(slots) == 0:
            return
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        w = self.state.view(torch.int32)
        w[idx, 7] = w[idx, 7] | _lib.NS_ST_DONE

    def compact(self, keep: Sequence[int]) -> None:
        """Keep rows ``keep`` (in that order) of every per-stream buffer: the session now has len(keep) streams."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(keep, dtype=np.int64), device=self.state.device)
        for name in ("payload", "nbits", "state", "out_token", "hist", "stats_acc", "trace", "qtable"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.index_select(0, idx).contiguous())
        self.nbits_host = self.nbits_host[np.asarray(keep, dtype=np.int64)]
        self.B = len(keep)

    def raise_errors(self) -> None:
        f = self.fields()["flags"]
        bad = np.nonzero(f & _lib.NS_ST_ERR_RANGE)[0]
        if bad.size:
            raise ArithmeticRangeError(f"streams {bad.tolist()[:8]} found no CDF bucket for the payload index")

    def tokens(self) -> List[List[int]]:
        self.raise_errors()
        f = self.fields()
        if int(f["ntokens"].max(initial=0)) > self.hist.shape[1]:
            raise ConfigurationError("token history overflow: raise max_tokens")
        return _rows_to_lists(self.hist, f["ntokens"])

    def trace_rows(self) -> np.ndarray:
        """Last-step trace as a structured host array (k, kprime, sel, n, token, exact, S)."""
        raw = self.trace.cpu().numpy()
        w = raw.view(np.int32).reshape(self.B, 8)
        return np.rec.fromarrays([w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 4], w[:, 5], raw[:, 3].view(np.float64)],
                                 names="k,kprime,sel,n,token,exact,S")


class DecodeSession:
    """B received token streams (ragged) being decoded back to bits."""

    def __init__(self, ctx: CoderContext, token_lists: Sequence[Sequence[int]],
                 quality: Optional[StreamQuality] = None):
        torch = _torch()
        self.ctx = ctx
        self.B = len(token_lists)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        _check_quality(ctx, self.B, quality)
        dev = torch.device("cuda", ctx.device)
        self.qtable = quality.table(dev) if quality is not None else None
        self.k_max = quality.k_max if quality is not None else 0
        self.lens = np.asarray([len(t) for t in token_lists], dtype=np.int64)
        self.T = int(self.lens.max(initial=0))
        tok = np.zeros((max(self.T, 1), self.B), dtype=np.int32)
        last = np.zeros((max(self.T, 1), self.B), dtype=np.uint8)
        act = np.zeros((max(self.T, 1), self.B), dtype=np.uint8)
        for i, tl in enumerate(token_lists):
            n = len(tl)
            if n:
                tok[:n, i] = np.asarray(tl, dtype=np.int32)
                last[n - 1, i] = 1
                act[:n, i] = 1
        self.tok = torch.from_numpy(tok).to(dev)
        self.last = torch.from_numpy(last).to(dev)
        self.act = torch.from_numpy(act).to(dev)
        P = quality.max_precision if quality is not None else ctx.params.precision  # the call's largest
        self.out_stride = int((self.T * P + P + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        self.state = _state_tensor(self.B, dev)
        with _table_registered(ctx, self.qtable, self.k_max):
            ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.trace = None
        self.t = 0

    def enable_trace(self):
        torch = _torch()
        self.trace = torch.zeros((self.B, 4), dtype=torch.int64, device=self.state.device)
        return self.trace

    def step(self, logits, *, force_exact: bool = False) -> None:
        p = self.ctx.params
        if self.t >= self.T:
            raise ConfigurationError("all tokens already decoded")
        t = self.t
        _check_logits(self.ctx, self.B, logits)
        flags = _lib.NS_STEP_FORCE_EXACT_SUM if force_exact else 0
        with _table_registered(self.ctx, self.qtable, self.k_max):
            rc = _lib.lib().ns_decode_step(
                self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.tok[t]), _ptr(self.last[t]),
                _ptr(self.act[t]), _ptr(self.state), _ptr(self.out_bits), self.out_stride, float(p.temp),
                int(p.topk), self.ctx._banned, self.ctx._nbanned, _ptr(self.trace), flags, _stream_handle())
        self.ctx.check(rc, "ns_decode_step")
        self.t += 1

    def step_static(self, logits, *, force_exact: bool = False):
        """:meth:`step` with the token index on the device (``d_t``): the step's token / last / active rows are
        gathered into fixed buffers by the device, so one captured hipGraph serves every step.  Returns the
        token buffer (the LM's next input)."""
        torch = _torch()
        _check_logits(self.ctx, self.B, logits)
        if getattr(self, "d_t", None) is None:
            self.d_t = torch.full((1,), self.t, dtype=torch.long, device=self.state.device)
            self.tok_s = torch.empty((1, self.B), dtype=self.tok.dtype, device=self.state.device)
            self.last_s = torch.empty((1, self.B), dtype=self.last.dtype, device=self.state.device)
            self.act_s = torch.empty((1, self.B), dtype=self.act.dtype, device=self.state.device)
        torch.index_select(self.tok, 0, self.d_t, out=self.tok_s)
        torch.index_select(self.last, 0, self.d_t, out=self.last_s)
        torch.index_select(self.act, 0, self.d_t, out=self.act_s)
        p = self.ctx.params
        flags = _lib.NS_STEP_FORCE_EXACT_SUM if force_exact else 0
        with _table_registered(self.ctx, self.qtable, self.k_max):
            rc = _lib.lib().ns_decode_step(
                self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.tok_s), _ptr(self.last_s),
                _ptr(self.act_s), _ptr(self.state), _ptr(self.out_bits), self.out_stride, float(p.temp),
                int(p.topk), self.ctx._banned, self.ctx._nbanned, _ptr(self.trace), flags, _stream_handle())
        self.ctx.check(rc, "ns_decode_step")
        self.d_t += 1
        return self.tok_s[0]

    def bits(self) -> List[List[int]]:
        f = _state_fields(self.state)
        bad = np.nonzero(f["flags"] & _lib.NS_ST_ERR_DIVERGE)[0]
        if bad.size:
            raise DecodeDivergenceError(f"streams {bad.tolist()[:8]}: received token outside the kept top-k")
        return _bit_rows_to_lists(self.out_bits, f["bit_pos"])


def encode_batch(ctx: CoderContext, payload_bits: Sequence[Sequence[int]], logits_fn, *, max_steps: int = 1 << 20,
                 check_every: int = 32, force_exact: bool = False, finish_sent: bool = False,
                 return_stats: bool = False, quality: Optional[StreamQuality] = None):
    """Run encode steps until every stream has consumed its payload; ``logits_fn(step, last_tokens)``
    returns the ``[B, ld]`` logits of that step.  ``return_stats=True`` returns ``(tokens, stats)`` with the
    per-stream statistics of ``encode_arithmetic`` (see :meth:`EncodeSession.stats`).  ``quality``: one row per
    stream (:class:`StreamQuality`) instead of the context's one quality."""
    sess = EncodeSession(ctx, payload_bits, stats=return_stats, quality=quality)
    last = sess.out_token
    for t in range(max_steps):
        if t % check_every == 0:
            if sess.all_done():
                break
            sess.ensure_history(check_every)
        last = sess.step(logits_fn(t, last), force_exact=force_exact, finish_sent=finish_sent)
    else:
        raise ConfigurationError("encode did not finish within max_steps")
    if return_stats:
        return sess.tokens(), sess.stats()
    return sess.tokens()


def decode_batch(ctx: CoderContext, token_lists: Sequence[Sequence[int]], logits_fn, *,
                 force_exact: bool = False, quality: Optional[StreamQuality] = None) -> List[List[int]]:
    sess = DecodeSession(ctx, token_lists, quality=quality)
    for t in range(sess.T):
        sess.step(logits_fn(t, sess.tok[t]), force_exact=force_exact)
    return sess.bits()


def sample_draw_rows(seeds: Sequence[int], gids: Sequence[int], lengths: Sequence[int]) -> np.ndarray:
    """``ns_sample_draw`` rows as [n, 4] int64 (the 32-byte rows as the device table holds them): seed (taken
    modulo 2^64), draw id, length (int32, the reserved words after it zero)."""
    n = len(seeds)
    if len(gids) != n or len(lengths) != n:
        raise ConfigurationError("one seed, one draw id and one length per stream")
    if any(int(v) < 0 or int(v) >= 1 << 31 for v in lengths):
        raise ConfigurationError("a stream's length must be within [0, 2^31)")
    rows = np.zeros((n, 4), dtype=np.int64)
    rows[:, 0] = np.asarray([int(s) & ((1 << 64) - 1) for s in seeds], dtype=np.uint64).view(np.int64)
    rows[:, 1] = np.asarray([int(g) for g in gids], dtype=np.int64)
    rows[:, 2] = np.asarray([int(v) for v in lengths], dtype=np.int64)
    return rows


class SampleSession:
    """B independent non-stego sampling streams (``code_base/sample.py:22-48``), one HIP launch per token.

    Draws are counter based (``ns_sample_step``): token t of stream b uses splitmix64(seed, stream_offset + b,
    t), so a run is reproducible and shardable (a rank passes its first global stream id as
    ``stream_offset``).  ``topk <= 0`` samples from every id.  Statistics (avg_NLL, avg_KL, avg_Hq of
    ``sample()``) are accumulated on the device when ``stats=True``.

    With ``quality`` (one :class:`StreamQuality` row per stream; its precision is not used) and ``seeds``, ``gids``,
    ``lengths`` (one each per stream) the session runs ``ns_sample_step_streams`` instead: stream b has its own
    temperature and top-k, draws token t with splitmix64(seeds[b], gids[b], t) whatever row it is in, and is parked
    -- nothing of it written -- once it has ``lengths[b]`` tokens.  ``seed``, ``topk``, ``temp`` and
    ``stream_offset`` are then not used.  Such a session also has the slot operations of :class:`EncodeSession`
    (:meth:`load_slots`, :meth:`park_slots`, :meth:`compact`, :meth:`harvest`)."""

    def __init__(self, ctx: CoderContext, B: int, *, seed: int = 0, topk: int = -1, temp: float = 1.0,
                 stream_offset: int = 0, max_tokens: int = 1024, stats: bool = True,
                 quality: Optional[StreamQuality] = None, seeds: Optional[Sequence[int]] = None,
                 gids: Optional[Sequence[int]] = None, lengths: Optional[Sequence[int]] = None):
        torch = _torch()
        if B < 1 or B > ctx.max_batch:
            raise ConfigurationError(f"batch {B} outside [1, {ctx.max_batch}]")
        if not temp > 0:
            raise ConfigurationError("temperature must be positive")
        self.ctx, self.B = ctx, int(B)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.topk, self.temp, self.stream_offset = int(topk), float(temp), int(stream_offset)
        dev = torch.device("cuda", ctx.device)
        self.qtable = self.draws = None
        self.k_max = 0
        if quality is not None:
            if seeds is None or gids is None or lengths is None:
                raise ConfigurationError("per-stream quality rows go with per-stream seeds, gids and lengths")
            _check_quality(ctx, self.B, quality)
            rows = sample_draw_rows(seeds, gids, lengths)
            if rows.shape[0] != self.B:
                raise ConfigurationError(f"{rows.shape[0]} draw rows for {self.B} streams")
            self.qtable, self.k_max = quality.table(dev), quality.k_max
            self.draws = torch.from_numpy(rows).to(dev)
            self.state = quality.init_rows(dev)
        elif seeds is not None or gids is not None or lengths is not None:
            raise ConfigurationError("per-stream seeds, gids and lengths go with per-stream quality rows")
        else:
            self.state = _state_tensor(self.B, dev)
            ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.hist = torch.full((self.B, int(max_tokens)), -1, dtype=torch.int32, device=dev)
        self.stats_acc = torch.zeros((self.B, 4), dtype=torch.float64, device=dev) if stats else None
        self.trace = None
        self.steps = 0

    def enable_trace(self):
        torch = _torch()
        self.trace = torch.zeros((self.B, 4), dtype=torch.int64, device=self.state.device)
        return self.trace

    def step(self, logits, *, diag_flags: int = 0):
        _check_logits(self.ctx, self.B, logits)
        if self.draws is not None:  # a stream ends at its own length (at most the history's width: load_slots)
            rc = _lib.lib().ns_sample_step_streams(
                self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.qtable), _ptr(self.draws),
                int(self.k_max), _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), self.hist.shape[1],
                self.ctx._banned, self.ctx._nbanned, _ptr(self.stats_acc), _ptr(self.trace), int(diag_flags),
                _stream_handle())
            self.ctx.check(rc, "ns_sample_step_streams")
            self.steps += 1
            return self.out_token
        if self.steps >= self.hist.shape[1]:
            raise ConfigurationError("token history full: raise max_tokens")
        rc = _lib.lib().ns_sample_step(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, ctypes.c_uint64(self.seed), self.stream_offset,
            _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), self.hist.shape[1], self.temp, self.topk,
            self.ctx._banned, self.ctx._nbanned, _ptr(self.stats_acc), _ptr(self.trace), int(diag_flags),
            _stream_handle())
        self.ctx.check(rc, "ns_sample_step")
        self.steps += 1
        return self.out_token

    def trace_rows(self) -> np.ndarray:
        t = self.trace.cpu().numpy().view(np.int32).reshape(self.B, 8)
        return np.rec.fromarrays([t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4]], names="k,kprime,sel,n,token")

    def tokens(self) -> List[List[int]]:
        if self.draws is not None:  # every stream's own count (at most its length)
            nt = _state_fields(self.state)["ntokens"]
            return _rows_to_lists(self.hist, np.minimum(nt, self.hist.shape[1]))
        n = min(self.steps, self.hist.shape[1])
        return _rows_to_lists(self.hist, np.full(self.B, n))

    # ---------------------------------------------------------------- slots (lm/slots.py: refill, compaction)
    def _tables(self) -> None:
        if self.draws is None:
            raise ConfigurationError("slot operations need a session created with per-stream tables")

    def load_slots(self, slots: Sequence[int], quality: StreamQuality, seeds: Sequence[int], gids: Sequence[int],
                   lengths: Sequence[int]) -> None:
        """Start new streams in ``slots`` (rows of this session): their quality and draw rows, a fresh state
        (``ntokens`` 0) and, with stats, zeroed accumulators.  The token history row is reused from position 0, and
        the history is widened first when an admitted length does not fit it."""
        self._tables()
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        if len(quality) != n or quality.k_max != self.k_max:
            raise ConfigurationError("load_slots: one quality row per slot, filled for the session's k_max")
        rows = sample_draw_rows(seeds, gids, lengths)
        if rows.shape[0] != n:
            raise ConfigurationError("load_slots: one draw row per slot")
        dev = self.state.device
        need = int(rows[:, 2].max())
        if need > self.hist.shape[1]:
            new = torch.full((self.B, need), -1, dtype=torch.int32, device=dev)
            new[:, : self.hist.shape[1]] = self.hist
            self.hist = new
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.qtable[idx] = quality.table(dev)
        self.draws[idx] = torch.from_numpy(rows).to(dev)
        self.state[idx] = quality.init_rows(dev)
        if self.stats_acc is not None:
            self.stats_acc[idx] = 0

    def park_slots(self, slots: Sequence[int]) -> None:
        """Park ``slots`` (length 0 in their draw rows): the step writes nothing for them."""
        self._tables()
        if len(slots) == 0:
            return
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        self.draws[idx, 2] = 0

    def compact(self, keep: Sequence[int]) -> None:
        """Keep rows ``keep`` (in that order) of every per-stream buffer: the session now has len(keep) streams."""
        self._tables()
        torch = _torch()
        idx = torch.as_tensor(np.asarray(keep, dtype=np.int64), device=self.state.device)
        for name in ("state", "out_token", "hist", "stats_acc", "trace", "qtable", "draws"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.index_select(0, idx).contiguous())
        self.B = len(keep)

    def harvest(self, slots: Sequence[int], lengths: Sequence[int]):
        """``(token lists, [n, 4] accumulators or None)`` of ``slots``, whose streams have reached ``lengths``."""
        self._tables()
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        toks = _rows_to_lists(self.hist.index_select(0, idx), lengths)
        acc = self.stats_acc.index_select(0, idx).cpu().numpy() if self.stats_acc is not None else None
        return toks, acc

    def stats(self) -> List[dict]:
        if self.stats_acc is None:
            raise ConfigurationError("the session was created without stats=True")
        return _stats_rows(self.stats_acc.cpu().numpy())


def sample_batch(ctx: CoderContext, B: int, length: int, logits_fn, *, seed: int, topk: int, temp: float,
                 stream_offset: int = 0, stats: bool = True):
    """``length`` sampler steps for B streams; ``logits_fn(step, last_tokens)`` returns the ``[B, ld]``
    logits.  Returns ``(tokens, stats)`` (stats None when ``stats=False``)."""
    sess = SampleSession(ctx, B, seed=seed, topk=topk, temp=temp, stream_offset=stream_offset,
                         max_tokens=max(1, length), stats=stats)
    last = sess.out_token
    for t in range(length):
        last = sess.step(logits_fn(t, last))
    return sess.tokens(), (sess.stats() if stats else None)


class StreamingDecodeSession:
    """Decode with the received tokens supplied step by step by the host (``code_base/arithmetic.py:254-371``
    loop, where the token list can change mid-stream: the BPE repair of ``:300-342`` inserts and deletes
    tokens).  A stream whose token falls outside the kept top-k' is flagged NS_ST_ERR_DIVERGE with its state
    untouched and its ranked kept ids exported; :meth:`clear` re-arms it for a re-issued step."""

    def __init__(self, ctx: CoderContext, B: int, max_tokens: int, quality: Optional[StreamQuality] = None):
        torch = _torch()
        if B < 1 or B > ctx.max_batch:
            raise ConfigurationError(f"batch {B} outside [1, {ctx.max_batch}]")
        self.ctx, self.B = ctx, int(B)
        _check_quality(ctx, self.B, quality)
        dev = torch.device("cuda", ctx.device)
        self.dev = dev
        self.qtable = quality.table(dev) if quality is not None else None
        self.k_max = quality.k_max if quality is not None else 0
        P = self.P = quality.max_precision if quality is not None else ctx.params.precision
        self.out_stride = int((max(1, max_tokens) * P + P + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        self.state = _state_tensor(self.B, dev)
        with _table_registered(ctx, self.qtable, self.k_max):
            ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.rank_stride = int(ctx.K) + 1
        self.ranked = torch.full((self.B, self.rank_stride), -1, dtype=torch.int32, device=dev)

    def _grow(self, need_bits: int) -> None:
        torch = _torch()
        need = (need_bits + 7) // 8 + 8
        if need <= self.out_stride:
            return
        new = torch.zeros((self.B, max(need, 2 * self.out_stride)), dtype=torch.uint8, device=self.dev)
        new[:, : self.out_stride] = self.out_bits
        self.out_bits, self.out_stride = new, new.shape[1]

    def step(self, logits, tokens: Sequence[int], is_last: Sequence[bool], active: Sequence[bool]) -> None:
        torch = _torch()
        p = self.ctx.params
        _check_logits(self.ctx, self.B, logits)
        f = _state_fields(self.state)
        self._grow(int(f["bit_pos"].max(initial=0)) + 2 * self.P)
        tok = torch.tensor(np.asarray(tokens, dtype=np.int32), device=self.dev)
        last = torch.tensor(np.asarray(is_last, dtype=np.uint8), device=self.dev)
        act = torch.tensor(np.asarray(active, dtype=np.uint8), device=self.dev)
        L = _lib.lib()
        self.ctx.check(L.ns_set_rank_export(self.ctx._h, _ptr(self.ranked), self.rank_stride), "ns_set_rank_export")
        with _table_registered(self.ctx, self.qtable, self.k_max):
            rc = L.ns_decode_step(self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(tok), _ptr(last), _ptr(act),
                                  _ptr(self.state), _ptr(self.out_bits), self.out_stride, float(p.temp), int(p.topk),
                                  self.ctx._banned, self.ctx._nbanned, ctypes.c_void_p(0), 0, _stream_handle())
        L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, "ns_decode_step")

    def diverged(self) -> List[int]:
        f = _state_fields(self.state)["flags"]
        return np.nonzero(f & _lib.NS_ST_ERR_DIVERGE)[0].tolist()

    def ranked_ids(self, b: int) -> List[int]:
        row = self.ranked[b].cpu().numpy()
        end = np.nonzero(row < 0)[0]
        return row[: int(end[0]) if end.size else row.size].astype(np.int64).tolist()

    def clear(self, streams: Sequence[int]) -> None:
        """Drop the divergence / done flags of ``streams`` (their lo/hi/bit_pos were left untouched)."""
        if not streams:
            return
        torch = _torch()
        w = self.state.view(torch.int32)
        idx = torch.tensor(list(streams), device=self.dev, dtype=torch.long)
        keep = ~(_lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE)
        w[idx, 7] = w[idx, 7] & keep

    def bits(self) -> List[List[int]]:
        f = _state_fields(self.state)
        return _bit_rows_to_lists(self.out_bits, f["bit_pos"])


class DecodeStreamsSession:
    """S slots of the arithmetic decoder with one quality row and one token row each (``ns_decode_step_streams``).

    A slot holds its stream's received tokens; a step decodes, for every slot, the token at the slot's own index --
    the stream's ``ntokens`` -- and stores the stream's bit count after that token in ``counts`` (the bit-count
    history a span search needs).  A slot past its last token, or flagged ``NS_ST_DONE`` (a divergence: state and bits
    untouched, its ranked ids in ``ranked``), is parked: nothing of it is written, so the loop may run steps without a
    host check.  Every buffer is sized at construction from ``max_tokens`` and ``max_precision`` (the call's largest):
    :meth:`step` reads nothing back, grows nothing and launches with fixed pointers, so a graph can replay it.  Every
    slot starts parked on a valid row."""

    def __init__(self, ctx: CoderContext, S: int, *, max_tokens: int, k_max: Optional[int] = None,
                 max_precision: Optional[int] = None, rank_export: bool = True):
        torch = _torch()
        self.ctx, self.B = ctx, int(S)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        if ctx.params.dtype == "f64":
            raise ConfigurationError("provider probability rows have no arithmetic decode step")
        self.k_max = int(k_max) if k_max is not None else int(ctx.params.topk)
        if self.k_max < 1 or self.k_max > ctx.params.topk:
            raise ConfigurationError("the coder context's topk must cover the session's k_max")
        self.P = int(max_precision) if max_precision is not None else int(ctx.params.precision)
        if not 1 <= self.P <= 60:
            raise ConfigurationError("precision must be within [1, 60]")
        dev = torch.device("cuda", ctx.device)
        self.T = max(1, int(max_tokens))
        self.tokmat = torch.zeros((self.B, self.T), dtype=torch.int32, device=dev)
        self.nlen = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.B, self.T), dtype=torch.int64, device=dev)
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        # a token emits at most `precision` bits (the last one exactly that many)
        self.out_stride = int((self.T * self.P + self.P + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        p = ctx.params
        filler = StreamQuality([CoderParams(vocab=p.vocab, precision=self.P, temp=1.0, topk=1, dtype=p.dtype,
                                            banned=p.banned)], k_max=self.k_max)
        self.qtable = filler.table(dev).expand(self.B, 4).contiguous()
        self.state = filler.init_rows(dev).expand(self.B, 4).contiguous()
        self.rank_stride = int(min(self.k_max, ctx.K)) + 1
        self.ranked = torch.full((self.B, self.rank_stride), -1, dtype=torch.int32, device=dev) if rank_export \
            else None
        self.trace = None
        self.steps = 0

    def enable_trace(self):
        self.trace = _state_tensor(self.B, self.state.device)
        return self.trace

    def step(self, logits, *, force_exact: bool = False):
        """One decode step for every slot; returns the out-token buffer ([B] int32: the token each stream consumed,
        the LM's next input; a parked stream keeps its last value)."""
        _check_logits(self.ctx, self.B, logits)
        L = _lib.lib()
        if self.ranked is not None:
            self.ctx.check(L.ns_set_rank_export(self.ctx._h, _ptr(self.ranked), self.rank_stride), "ns_set_rank_export")
        rc = L.ns_decode_step_streams(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.qtable), int(self.k_max), _ptr(self.tokmat),
            self.T, _ptr(self.nlen), _ptr(self.state), _ptr(self.out_bits), self.out_stride, _ptr(self.counts), self.T,
            _ptr(self.out_token), self.ctx._banned, self.ctx._nbanned, _ptr(self.trace),
            _lib.NS_STEP_FORCE_EXACT_SUM if force_exact else 0, _stream_handle())
        if self.ranked is not None:
            L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, "ns_decode_step_streams")
        self.steps += 1
        return self.out_token

    # ---------------------------------------------------------------- slots (lm/slots.py: refill, compaction)
    def load_slots(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], quality: StreamQuality) -> None:
        """Start new streams in ``slots``: their tokens and count, their quality row, a fresh state (``ntokens`` 0,
        ``hi = 2^precision`` of the row) and zeroed output bytes and counts."""
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        if quality is None or len(quality) != n or len(token_lists) != n or quality.k_max != self.k_max:
            raise ConfigurationError("load_slots: one token list and one quality row per slot, filled for the "
                                     "session's k_max")
        if quality.max_precision > self.P:
            raise ConfigurationError("load_slots: a row's precision exceeds the one the session was sized for")
        tok = np.zeros((n, self.T), dtype=np.int32)
        nl = np.zeros(n, dtype=np.int32)
        for i, tl in enumerate(token_lists):
            k = len(tl)
            if k > self.T:
                raise ConfigurationError("stream longer than the session was sized for")
            tok[i, :k] = np.asarray(tl, dtype=np.int32)
            nl[i] = k
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.tokmat[idx] = torch.from_numpy(tok).to(dev)
        self.nlen[idx] = torch.from_numpy(nl).to(dev)
        self.qtable[idx] = quality.table(dev)
        self.state[idx] = quality.init_rows(dev)
        self.out_bits[idx] = 0
        self.counts[idx] = 0

    def park_slots(self, slots: Sequence[int]) -> None:
        """Park ``slots`` (token count 0): the step writes nothing for them."""
        if len(slots) == 0:
            return
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        self.nlen[idx] = 0

    def compact(self, keep: Sequence[int]) -> None:
        """Keep rows ``keep`` (in that order) of every per-stream buffer: the session now has len(keep) streams."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(keep, dtype=np.int64), device=self.state.device)
        for name in ("tokmat", "nlen", "counts", "out_token", "out_bits", "qtable", "state", "ranked", "trace"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.index_select(0, idx).contiguous())
        self.B = len(keep)

    def clear(self, slots: Sequence[int], tokens: Optional[Sequence[int]] = None) -> None:
        """Re-arm diverged ``slots``: drop their divergence / done flags (state and bits were left untouched) and,
        with ``tokens``, replace the token each of them diverged on."""
        if len(slots) == 0:
            return
        torch = _torch()
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        w = self.state.view(torch.int32)
        w[idx, 7] = w[idx, 7] & ~(_lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE)
        if tokens is not None:
            at = w[idx, 6].long().clamp(0, self.T - 1)
            self.tokmat[idx, at] = torch.as_tensor(np.asarray(tokens, dtype=np.int32), device=dev)

    def harvest(self, slots: Sequence[int]):
        """``(bits, counts, flags, ntokens)`` of ``slots``: per slot the decoded bit list (``bit_pos`` bits), the bit
        count after each of its ``ntokens`` decoded tokens, its state flags and ``ntokens``."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        f = _state_fields(self.state.index_select(0, idx))
        nt = np.minimum(f["ntokens"].astype(np.int64), self.T)
        bits = _bit_rows_to_lists(self.out_bits.index_select(0, idx), f["bit_pos"])
        counts = _rows_to_lists(self.counts.index_select(0, idx), nt)
        return bits, counts, f["flags"].copy(), nt

    def ranked_ids(self, b: int) -> List[int]:
        row = self.ranked[b].cpu().numpy()
        end = np.nonzero(row < 0)[0]
        return row[: int(end[0]) if end.size else row.size].astype(np.int64).tolist()


def rank_quality(quality) -> "_lib.NsRankQuality":
    """src codec quality (``lm/arithmetic.py:77-95`` ``_normalise_quality``: topk/top_k, top_p, min_prob,
    cap_per_token_bits / cap_bits_per_token) -> ``ns_rank_quality``."""
    q = {}
    for key, value in dict(quality or {}).items():
        if value is None:
            continue
        k = key.replace("-", "_").lower()
        if k in ("topk", "top_k"):
            q["top_k"] = int(value)
        elif k in ("topp", "top_p"):
            q["top_p"] = float(value)
        elif k in ("minprob", "min_prob"):
            q["min_prob"] = float(value)
        elif k in ("cap_per_token_bits", "cap_bits_per_token"):
            q["cap"] = int(value)
        elif k == "prob_temp":  # crypto quality LM (crypto/quality.py:57-64): temperature on probabilities
            q["prob_temp"] = float(value)
    if "top_k" in q and q["top_k"] <= 0:
        raise ConfigurationError("top_k must be positive")
    if "top_p" in q and not 0 < q["top_p"] <= 1:
        raise ConfigurationError("top_p must be within (0, 1]")
    if "min_prob" in q and q["min_prob"] < 0:
        raise ConfigurationError("min_prob must be non-negative")
    if "cap" in q and q["cap"] <= 0:
        raise ConfigurationError("cap_per_token_bits must be positive")
    if "prob_temp" in q and q["prob_temp"] <= 0:
        raise ConfigurationError("temperature must be positive")
    if "prob_temp" in q and ("cap" in q or "min_prob" in q):
        raise ConfigurationError("the crypto quality policy takes only top_k, top_p and temperature")
    return _lib.NsRankQuality(q.get("top_k", 0), q.get("cap", 0), q.get("top_p", 0.0), q.get("min_prob", -1.0),
                              q.get("prob_temp", 0.0))


def _rank_trace_rows(trace, B: int) -> np.ndarray:
    """A rank session's last-step trace as a structured host array: ``k`` the support size n, ``kprime`` the capacity
    c = floor(log2 n), ``sel`` the rank, ``n`` the bits taken (encode) or kept (decode), ``token``, ``S``.  A stream
    that took no step in the launch (finished, inactive or in error) keeps its previous row."""
    if trace is None:
        raise ConfigurationError("the session's trace is off: call enable_trace() first")
    raw = trace.cpu().numpy()
    w = raw.view(np.int32).reshape(B, 8)
    return np.rec.fromarrays([w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 4], raw[:, 3].view(np.float64)],
                             names="k,kprime,sel,n,token,S")


class RankEncodeSession:
    """B payloads (bytes) encoded by the src rank coder (``codec/arithmetic.py:122-168``), one launch per
    token; :meth:`consumed` is the reference's ``state["history"]`` per stream."""

    def __init__(self, ctx: CoderContext, payloads: Sequence[bytes], *, temp: float, quality=None,
                 max_tokens: Optional[int] = None):
        torch = _torch()
        self.ctx, self.B = ctx, len(payloads)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        dev = torch.device("cuda", ctx.device)
        self.temp, self.q = float(temp), rank_quality(quality)
        self.nbytes = [len(bytes(pl)) for pl in payloads]
        stride = max(1, max(self.nbytes))
        buf = np.zeros((self.B, stride), dtype=np.uint8)
        for i, pl in enumerate(payloads):
            buf[i, : len(pl)] = np.frombuffer(bytes(pl), dtype=np.uint8)
        self.payload = torch.from_numpy(buf).to(dev)
        self.nbits = torch.tensor([8 * n for n in self.nbytes], dtype=torch.int64, device=dev)
        self.state = _state_tensor(self.B, dev)
        ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        cap = max_tokens if max_tokens is not None else 8 * stride + 16
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.hist = torch.full((self.B, cap), -1, dtype=torch.int32, device=dev)
        self.cons = torch.zeros((self.B, cap), dtype=torch.int32, device=dev)
        self.trace = None

    def enable_trace(self):
        """Have every step write its ``ns_step_trace`` row per stream (see :func:`_rank_trace_rows`)."""
        self.trace = _state_tensor(self.B, self.state.device)
        return self.trace

    def trace_rows(self) -> np.ndarray:
        return _rank_trace_rows(self.trace, self.B)

    def step(self, logits):
        logits = _rank_rows(self.ctx, self.B, logits, self.q)
        rc = _lib.lib().ns_rank_encode_step(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.payload), self.payload.stride(0),
            _ptr(self.nbits), _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), _ptr(self.cons),
            self.hist.shape[1], self.temp, ctypes.byref(self.q), _ptr(self.trace), 0, _stream_handle())
        self.ctx.check(rc, "ns_rank_encode_step")
        return self.out_token

    def fields(self) -> dict:
        return _state_fields(self.state)

    def all_done(self) -> bool:
        f = self.fields()
        return bool(np.all((f["flags"] & _lib.NS_ST_DONE) != 0))

    def raise_errors(self) -> None:
        bad = np.nonzero(self.fields()["flags"] & _lib.NS_ST_ERR_RANGE)[0]
        if bad.size:
            raise ArithmeticRangeError(f"streams {bad.tolist()[:8]}: language model distribution provides no capacity")

    def tokens(self) -> List[List[int]]:
        self.raise_errors()
        n = self.fields()["ntokens"]
        h = self.hist.cpu().numpy()
        return [h[i, : int(n[i])].astype(np.int64).tolist() for i in range(self.B)]

    def consumed(self) -> List[List[int]]:
        n = self.fields()["ntokens"]
        c = self.cons.cpu().numpy()
        return [c[i, : int(n[i])].astype(np.int64).tolist() for i in range(self.B)]


class RankDecodeSession:
    """Decode of the rank coder (``codec/arithmetic.py:171-231``) given every stream's consumption history."""

    def __init__(self, ctx: CoderContext, token_lists: Sequence[Sequence[int]], histories: Sequence[Sequence[int]],
                 *, temp: float, quality=None):
        torch = _torch()
        self.ctx, self.B = ctx, len(token_lists)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        for tl, hs in zip(token_lists, histories):
            if len(hs) < len(tl):
                raise DecodeDivergenceError("Bit consumption history is required for decoding")
        dev = torch.device("cuda", ctx.device)
        self.temp, self.q = float(temp), rank_quality(quality)
        self.T = max((len(t) for t in token_lists), default=0)
        T1 = max(self.T, 1)
        tok = np.zeros((T1, self.B), np.int32)
        keep = np.zeros((T1, self.B), np.int32)
        act = np.zeros((T1, self.B), np.uint8)
        for i, (tl, hs) in enumerate(zip(token_lists, histories)):
            n = len(tl)
            tok[:n, i] = np.asarray(tl, np.int32)
            keep[:n, i] = np.asarray(list(hs)[:n], np.int32)
            act[:n, i] = 1
        self.tok, self.keep, self.act = (torch.from_numpy(a).to(dev) for a in (tok, keep, act))
        total = int(max((sum(list(h)[: len(t)]) for t, h in zip(token_lists, histories)), default=0))
        self.out_stride = (total + 7) // 8 + 8
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        self.state = _state_tensor(self.B, dev)
        ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.t = 0
        self.trace = None

    def enable_trace(self):
        """As :meth:`RankEncodeSession.enable_trace`; ``n`` is the number of bits kept of the token's rank."""
        self.trace = _state_tensor(self.B, self.state.device)
        return self.trace

    def trace_rows(self) -> np.ndarray:
        return _rank_trace_rows(self.trace, self.B)

    def step(self, logits) -> None:
        t = self.t
        logits = _rank_rows(self.ctx, self.B, logits, self.q)
        rc = _lib.lib().ns_rank_decode_step(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.tok[t]), _ptr(self.keep[t]),
            _ptr(self.act[t]), _ptr(self.state), _ptr(self.out_bits), self.out_stride, self.temp,
            ctypes.byref(self.q), _ptr(self.trace), 0, _stream_handle())
        self.ctx.check(rc, "ns_rank_decode_step")
        self.t += 1

    def payloads(self) -> List[bytes]:
        f = _state_fields(self.state)
        bad = np.nonzero(f["flags"] & _lib.NS_ST_ERR_DIVERGE)[0]
        if bad.size:
            raise DecodeDivergenceError(f"streams {bad.tolist()[:8]}: token not present in distribution")
        ob = self.out_bits.cpu().numpy()
        return [ob[i, : int(f["bit_pos"][i]) // 8].tobytes() for i in range(self.B)]


# ---------------------------------------------------------------------------------------------- rank coder, per stream
def _rank_temp(quality) -> float:
    """The softmax temperature of a rank quality mapping (``temp`` / ``temperature``, default 1), as the rank
    provider reads it."""
    for key in ("temp", "temperature"):
        if quality and quality.get(key) is not None:
            t = float(quality[key])
            if t <= 0:
                raise ConfigurationError("temperature must be positive")
            return t
    return 1.0


def rank_stream_quality_rows(qualities, temps: Optional[Sequence[float]] = None) -> np.ndarray:
    """``ns_rank_stream_quality`` rows as [n, 6] int64 (the 48-byte rows as the device table holds them), one per
    quality mapping: keys and errors of :func:`rank_quality`, the temperature from the mapping (``temp`` /
    ``temperature``) or from ``temps``; filled by the library's ``ns_rank_stream_quality_fill``."""
    qs = list(qualities)
    if temps is not None and len(temps) != len(qs):
        raise ConfigurationError("one temperature per quality")
    rows = np.zeros((len(qs), _lib.NS_RANK_STREAM_QUALITY_BYTES // 8), dtype=np.int64)
    L = _lib.lib()
    for i, q in enumerate(qs):
        rq = q if isinstance(q, _lib.NsRankQuality) else rank_quality(q)
        temp = float(temps[i]) if temps is not None else _rank_temp(None if isinstance(q, _lib.NsRankQuality) else q)
        row = _lib.NsRankStreamQuality()
        if L.ns_rank_stream_quality_fill(temp, ctypes.byref(rq), ctypes.byref(row)) != _lib.NS_OK:
            raise ConfigurationError(f"quality {i}: {L.ns_last_error(None).decode()}")
        rows[i] = np.frombuffer(bytes(row), dtype=np.int64)
    return rows


class RankStreamQuality:
    """One ``ns_rank_stream_quality`` row per message (:func:`rank_stream_quality_rows`), as the slot loops take
    them: :meth:`take` picks the rows of some messages, :meth:`table` puts them on a device."""

    def __init__(self, rows: np.ndarray):
        self.rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, _lib.NS_RANK_STREAM_QUALITY_BYTES // 8)

    @classmethod
    def from_qualities(cls, qualities, temps=None) -> "RankStreamQuality":
        return cls(rank_stream_quality_rows(qualities, temps))

    def __len__(self) -> int:
        return self.rows.shape[0]

    def take(self, idx: Sequence[int]) -> "RankStreamQuality":
        return RankStreamQuality(self.rows[np.asarray(list(idx), dtype=np.int64)])

    def table(self, device):
        return _torch().from_numpy(self.rows.copy()).to(device)


_RANK_OFF_ROW = None


def _rank_off_rows(n: int) -> RankStreamQuality:
    """``n`` valid rows (temperature 1, every policy off): what an empty slot holds."""
    global _RANK_OFF_ROW
    if _RANK_OFF_ROW is None:
        _RANK_OFF_ROW = rank_stream_quality_rows([{}])
    return RankStreamQuality(np.repeat(_RANK_OFF_ROW, n, axis=0))


class RankStreamEncodeSession:
    """S slots of the rank coder with one quality row each (``ns_rank_encode_step_streams``): the slot operations of
    :class:`EncodeSession` (:meth:`load_slots`, :meth:`park_slots`, :meth:`compact`, :meth:`ensure_history`) plus
    :meth:`harvest`.  Every slot starts parked (NS_ST_DONE, no payload) on a valid row; with ``payloads`` and
    ``quality`` the session starts with those streams loaded in slots 0..S-1."""

    stats_acc = None  # the rank coder accumulates no statistics

    def __init__(self, ctx: CoderContext, S: int, *, payload_stride: int = 1, max_tokens: int = 64,
                 payloads: Optional[Sequence[bytes]] = None, quality: Optional[RankStreamQuality] = None):
        torch = _torch()
        self.ctx, self.B = ctx, int(S)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        if ctx.params.dtype == "f64":
            raise ConfigurationError("provider probability rows take one quality per call (no per-stream table)")
        dev = torch.device("cuda", ctx.device)
        stride = max(1, int(payload_stride), max((len(p) for p in payloads), default=1) if payloads else 1)
        self.payload = torch.zeros((self.B, stride), dtype=torch.uint8, device=dev)
        self.nbits = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self.state = _state_tensor(self.B, dev)
        ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.qtable = _rank_off_rows(self.B).table(dev)
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        cap = max(1, int(max_tokens))
        self.hist = torch.full((self.B, cap), -1, dtype=torch.int32, device=dev)
        self.cons = torch.zeros((self.B, cap), dtype=torch.int32, device=dev)
        self.trace = None
        self.park_slots(np.arange(self.B))
        if payloads is not None:
            if quality is None or len(payloads) != self.B:
                raise ConfigurationError("one payload and one quality row per stream")
            need = 8 * stride + 16
            if need > cap:
                self.ensure_history(need)
            self.load_slots(np.arange(self.B), payloads, quality)

    def enable_trace(self):
        self.trace = _state_tensor(self.B, self.state.device)
        return self.trace

    def trace_rows(self) -> np.ndarray:
        return _rank_trace_rows(self.trace, self.B)

    def step(self, logits, *, finish_sent: bool = False):
        if finish_sent:
            raise ConfigurationError("the rank coder has no finish_sent")
        _check_logits(self.ctx, self.B, logits)
        rc = _lib.lib().ns_rank_encode_step_streams(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(self.payload), self.payload.stride(0),
            _ptr(self.nbits), _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), _ptr(self.cons),
            self.hist.shape[1], _ptr(self.qtable), _ptr(self.trace), 0, _stream_handle())
        self.ctx.check(rc, "ns_rank_encode_step_streams")
        return self.out_token

    def fields(self) -> dict:
        return _state_fields(self.state)

    def all_done(self) -> bool:
        return bool(np.all((self.fields()["flags"] & _lib.NS_ST_DONE) != 0))

    def raise_errors(self) -> None:
        bad = np.nonzero(self.fields()["flags"] & _lib.NS_ST_ERR_RANGE)[0]
        if bad.size:
            raise ArithmeticRangeError(f"streams {bad.tolist()[:8]}: language model distribution provides no capacity")

    def ensure_history(self, steps_ahead: int) -> None:
        """Grow the token and consumption histories so ``steps_ahead`` more steps fit."""
        need = int(self.fields()["ntokens"].max(initial=0)) + int(steps_ahead)
        cap = self.hist.shape[1]
        if need <= cap:
            return
        torch = _torch()
        width = max(need, 2 * cap)
        for name, fill in (("hist", -1), ("cons", 0)):
            old = getattr(self, name)
            new = torch.full((self.B, width), fill, dtype=torch.int32, device=old.device)
            new[:, :cap] = old
            setattr(self, name, new)

    def load_slots(self, slots: Sequence[int], payloads: Sequence[object], quality: RankStreamQuality) -> None:
        """Start new payloads in ``slots``: payload bytes (``bytes``, or the api's bit list -- LSB-first per byte, a
        multiple of 8 long), bit count, a fresh state and the stream's quality row.  The history rows are reused from
        position 0."""
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        if quality is None or len(quality) != n or len(payloads) != n:
            raise ConfigurationError("load_slots: one payload and one quality row per slot")
        stride = self.payload.shape[1]
        pl = np.zeros((n, stride), dtype=np.uint8)
        nb = np.zeros(n, dtype=np.int64)
        for i, p in enumerate(payloads):
            if isinstance(p, (bytes, bytearray)):
                packed = np.frombuffer(bytes(p), dtype=np.uint8)
            else:
                if len(p) % 8:
                    raise ConfigurationError("bit stream length must be a multiple of 8")
                packed = np.packbits(_bit_array(p) != 0, bitorder="little") if len(p) else np.zeros(0, np.uint8)
            if packed.size > stride:
                raise ConfigurationError("payload longer than the session's payload stride")
            pl[i, : packed.size] = packed
            nb[i] = 8 * packed.size
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.payload[idx] = torch.from_numpy(pl).to(dev)
        self.nbits[idx] = torch.from_numpy(nb).to(dev)
        self.qtable[idx] = quality.table(dev)
        self.state[idx] = torch.tensor([[0, 1 << self.ctx.params.precision, 0, 0]], dtype=torch.int64,
                                       device=dev).expand(n, 4)

    def park_slots(self, slots: Sequence[int]) -> None:
        """Mark ``slots`` finished (NS_ST_DONE): the step writes nothing for them; their rows stay valid."""
        if len(slots) == 0:
            return
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        w = self.state.view(torch.int32)
        w[idx, 7] = w[idx, 7] | _lib.NS_ST_DONE

    def compact(self, keep: Sequence[int]) -> None:
        """Keep rows ``keep`` (in that order) of every per-stream buffer: the session now has len(keep) streams."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(keep, dtype=np.int64), device=self.state.device)
        for name in ("payload", "nbits", "state", "out_token", "hist", "cons", "trace", "qtable"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.index_select(0, idx).contiguous())
        self.B = len(keep)

    def harvest(self, slots: Sequence[int]):
        """``(token lists, consumed-bit lists)`` of ``slots`` (finished streams: the reference's tokens and
        ``state["history"]``)."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        nt = _state_fields(self.state.index_select(0, idx))["ntokens"]
        return (_rows_to_lists(self.hist.index_select(0, idx), nt),
                _rows_to_lists(self.cons.index_select(0, idx), nt))

    def tokens(self) -> List[List[int]]:
        self.raise_errors()
        return self.harvest(np.arange(self.B))[0]

    def consumed(self) -> List[List[int]]:
        return self.harvest(np.arange(self.B))[1]


class RankStreamDecodeSession:
    """S slots of the rank decoder with one quality row each (``ns_rank_decode_step_streams``).  A slot holds its
    message's tokens and keep-bits (the consumption history); a step decodes, for every slot, the token at the
    slot's own index -- the stream's ``ntokens`` -- and a slot past its last token is inactive (nothing of it is
    written), so the loop may run steps without a host check.  Every slot starts empty on a valid row."""

    def __init__(self, ctx: CoderContext, S: int, *, max_tokens: int, max_bits: int,
                 token_lists: Optional[Sequence[Sequence[int]]] = None,
                 histories: Optional[Sequence[Sequence[int]]] = None, quality: Optional[RankStreamQuality] = None):
        torch = _torch()
        self.ctx, self.B = ctx, int(S)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        if ctx.params.dtype == "f64":
            raise ConfigurationError("provider probability rows take one quality per call (no per-stream table)")
        dev = torch.device("cuda", ctx.device)
        self.T = max(1, int(max_tokens))
        self.tokmat = torch.zeros((self.B, self.T), dtype=torch.int32, device=dev)
        self.keepmat = torch.zeros((self.B, self.T), dtype=torch.int32, device=dev)
        self.nlen = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.out_stride = (max(0, int(max_bits)) + 7) // 8 + 8
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        self.state = _state_tensor(self.B, dev)
        ctx.check(_lib.lib().ns_init_state(ctx._h, _ptr(self.state), self.B, _stream_handle()), "ns_init_state")
        self.qtable = _rank_off_rows(self.B).table(dev)
        self.trace = None
        self._bufs = {}
        if token_lists is not None:
            if histories is None or quality is None or len(token_lists) != self.B:
                raise ConfigurationError("one token list, one history and one quality row per stream")
            self.load_slots(np.arange(self.B), token_lists, histories, quality)

    def enable_trace(self):
        self.trace = _state_tensor(self.B, self.state.device)
        return self.trace

    def trace_rows(self) -> np.ndarray:
        return _rank_trace_rows(self.trace, self.B)

    def step(self, logits):
        """One decode step; returns the [B] tokens it fed (a slot past its end: its last token, inactive)."""
        torch = _torch()
        _check_logits(self.ctx, self.B, logits)
        tix = self.state.view(torch.int32)[:, 6]  # ntokens: the index of the stream's next token
        idx = tix.clamp(0, self.T - 1).long().unsqueeze(1)
        tok = torch.gather(self.tokmat, 1, idx).squeeze(1).contiguous()
        keep = torch.gather(self.keepmat, 1, idx).squeeze(1).contiguous()
        act = (tix < self.nlen).to(torch.uint8)
        self._bufs = {"tok": tok, "keep": keep, "act": act}  # alive until the next step (graph replays reuse them)
        rc = _lib.lib().ns_rank_decode_step_streams(
            self.ctx._h, _ptr(logits), logits.stride(0), self.B, _ptr(tok), _ptr(keep), _ptr(act), _ptr(self.state),
            _ptr(self.out_bits), self.out_stride, _ptr(self.qtable), _ptr(self.trace), 0, _stream_handle())
        self.ctx.check(rc, "ns_rank_decode_step_streams")
        return tok

    def load_slots(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]],
                   histories: Sequence[Sequence[int]], quality: RankStreamQuality) -> None:
        """Start new messages in ``slots``: tokens, keep-bits, token count, zeroed output bytes, a fresh state and
        the stream's quality row."""
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        if quality is None or len(quality) != n or len(token_lists) != n or len(histories) != n:
            raise ConfigurationError("load_slots: one token list, one history and one quality row per slot")
        tok = np.zeros((n, self.T), dtype=np.int32)
        keep = np.zeros((n, self.T), dtype=np.int32)
        nl = np.zeros(n, dtype=np.int32)
        for i, (tl, hs) in enumerate(zip(token_lists, histories)):
            k = len(tl)
            if len(hs) < k:
                raise DecodeDivergenceError("Bit consumption history is required for decoding")
            if k > self.T or sum(list(hs)[:k]) > 8 * (self.out_stride - 8):
                raise ConfigurationError("message longer than the session was sized for")
            tok[i, :k] = np.asarray(tl, dtype=np.int32)
            keep[i, :k] = np.asarray(list(hs)[:k], dtype=np.int32)
            nl[i] = k
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.tokmat[idx] = torch.from_numpy(tok).to(dev)
        self.keepmat[idx] = torch.from_numpy(keep).to(dev)
        self.nlen[idx] = torch.from_numpy(nl).to(dev)
        self.out_bits[idx] = 0
        self.qtable[idx] = quality.table(dev)
        self.state[idx] = torch.tensor([[0, 1 << self.ctx.params.precision, 0, 0]], dtype=torch.int64,
                                       device=dev).expand(n, 4)

    def park_slots(self, slots: Sequence[int]) -> None:
        """Empty ``slots`` (token count 0): the step leaves them inactive."""
        if len(slots) == 0:
            return
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        self.nlen[idx] = 0

    def compact(self, keep: Sequence[int]) -> None:
        torch = _torch()
        idx = torch.as_tensor(np.asarray(keep, dtype=np.int64), device=self.state.device)
        for name in ("tokmat", "keepmat", "nlen", "out_bits", "state", "trace", "qtable"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.index_select(0, idx).contiguous())
        self.B = len(keep)

    @staticmethod
    def payloads_of(state_rows, out_rows) -> List[bytes]:
        """The decoded bytes of host copies of some slots' state and output rows (whole bytes only, as
        :meth:`RankDecodeSession.payloads` returns them)."""
        f = _state_fields(state_rows)
        ob = out_rows.cpu().numpy()
        return [ob[i, : int(f["bit_pos"][i]) // 8].tobytes() for i in range(ob.shape[0])]

    def harvest(self, slots: Sequence[int]):
        """``(payload bytes, flags)`` of ``slots``."""
        torch = _torch()
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.state.device)
        st = self.state.index_select(0, idx)
        return self.payloads_of(st, self.out_bits.index_select(0, idx)), _state_fields(st)["flags"]

    def payloads(self) -> List[bytes]:
        pls, flags = self.harvest(np.arange(self.B))
        bad = np.nonzero(flags & _lib.NS_ST_ERR_DIVERGE)[0]
        if bad.size:
            raise DecodeDivergenceError(f"streams {bad.tolist()[:8]}: token not present in distribution")
        return pls


# ---------------------------------------------------------------------------------------------------------------
# Fixed-block baseline coders (include/nsg_baseline.h): code_base/huffman_baseline.py and code_base/block_baseline.py
# ---------------------------------------------------------------------------------------------------------------
BASELINE_MODES = ("huffman", "bins")


def bins_permutation(vocab_size: int, block_size: int) -> np.ndarray:
    """The vocabulary order ``block_baseline.get_bins`` shuffles (``np.random.seed(block_size)`` then
    ``np.random.shuffle``): the same MT19937 stream from a private ``RandomState``, so numpy's global generator
    is left alone."""
    order = np.arange(int(vocab_size))
    np.random.RandomState(int(block_size)).shuffle(order)
    return order


def bins_table(vocab_size: int, block_size: int) -> np.ndarray:
    """uint8[vocab]: the bin of every id (``words2bin`` of ``block_baseline.get_bins``, block_baseline.py:9-24)."""
    order = bins_permutation(vocab_size, block_size)
    num_bins = 2 ** int(block_size)
    words_per_bin = vocab_size / num_bins
    table = np.zeros(int(vocab_size), dtype=np.uint8)
    for j in range(num_bins):
        table[order[int(j * words_per_bin):int((j + 1) * words_per_bin)]] = j
    return table


class BaselineSpec:
    """One call's baseline coder: ``mode`` ("huffman" or "bins") and ``block_size`` (1..8, with 2**block_size ids
    left after the ban), checked against a context; holds the device word-to-bin table of the bins coder."""

    def __init__(self, ctx: CoderContext, mode: str, block_size: int, table=None):
        if mode not in BASELINE_MODES:
            raise ConfigurationError(f"mode must be one of {BASELINE_MODES}")
        self.mode = mode
        self.block = int(block_size)
        self.K = baseline_leaders(ctx.params.vocab, ctx.params.banned_ids(), block_size)
        if ctx.params.dtype not in ("f32", "f16"):
            raise ConfigurationError("the baseline coders take fp32 or fp16 logits rows")
        self.max_bits = self.K - 1 if mode == "huffman" else self.block  # bits one token can carry
        self.table = None
        if mode == "bins":
            torch = _torch()
            t = bins_table(ctx.params.vocab, self.block) if table is None else np.asarray(table, dtype=np.uint8)
            if t.shape != (ctx.params.vocab,) or int(t.max(initial=0)) >= self.K:
                raise ConfigurationError("the word-to-bin table needs one bin below 2**block_size per id")
            self.table = torch.from_numpy(np.ascontiguousarray(t)).to(torch.device("cuda", ctx.device))

    def entry(self, name: str):
        return getattr(_lib.lib(), f"ns_{self.mode}_{name}")

    def head(self, ctx: CoderContext, logits, B: int):
        """The leading arguments every baseline entry point shares."""
        args = [ctx._h, _ptr(logits), logits.stride(0), B, self.block]
        if self.mode == "bins":
            args.append(_ptr(self.table))
        return args


def baseline_leaders(vocab: int, banned: Sequence[int], block_size) -> int:
    """K = 2**block_size after the checks every baseline entry point makes."""
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or not 1 <= int(block_size) <= 8:
        raise ConfigurationError("block_size must be an integer within [1, 8]")
    valid = int(vocab) - len({int(b) for b in banned if 0 <= int(b) < int(vocab)})
    if (1 << int(block_size)) > valid:
        raise ConfigurationError(f"2**block_size = {1 << int(block_size)} exceeds the {valid} ids left after the ban")
    return 1 << int(block_size)


class BaselineEncodeSession(EncodeSession):
    """:class:`EncodeSession` of a baseline coder: the same payload, state, history and slot methods, one
    ``ns_huffman_encode_step`` / ``ns_bins_encode_step`` per :meth:`step`.  ``stats=True`` accumulates the
    reference's avg_NLL, avg_KL and words_per_bit (``avg_Hq`` has no counterpart and stays 0)."""

    def __init__(self, ctx: CoderContext, payload_bits: Sequence[Sequence[int]], *, mode: str, block_size: int,
                 max_tokens: Optional[int] = None, stats: bool = False, payload_stride: Optional[int] = None,
                 table=None):
        self.spec = BaselineSpec(ctx, mode, block_size, table)
        super().__init__(ctx, payload_bits, max_tokens=max_tokens, stats=stats, payload_stride=payload_stride)

    def step(self, logits, *, finish_sent: bool = False):
        self._check_logits(logits)
        flags = _lib.NS_STEP_FINISH_SENT if finish_sent else 0
        rc = self.spec.entry("encode_step")(
            *self.spec.head(self.ctx, logits, self.B), _ptr(self.payload), self.payload.stride(0), _ptr(self.nbits),
            _ptr(self.state), _ptr(self.out_token), _ptr(self.hist), self.hist.shape[1], self.ctx._banned,
            self.ctx._nbanned, _ptr(self.stats_acc), _ptr(self.trace), flags, _stream_handle())
        self.ctx.check(rc, f"ns_{self.spec.mode}_encode_step")
        self.steps += 1
        return self.out_token

    def raise_errors(self) -> None:
        f = self.fields()["flags"]
        bad = np.nonzero(f & _lib.NS_ST_ERR_RANGE)[0]
        if bad.size:
            raise ArithmeticRangeError(f"streams {bad.tolist()[:8]}: a row the {self.spec.mode} coder cannot code")


class BaselineDecodeSession(DecodeSession):
    """:class:`DecodeSession` of a baseline coder (lockstep: token t of every stream per step)."""

    def __init__(self, ctx: CoderContext, token_lists: Sequence[Sequence[int]], *, mode: str, block_size: int,
                 table=None):
        self.spec = BaselineSpec(ctx, mode, block_size, table)
        super().__init__(ctx, token_lists)
        torch = _torch()
        self.out_stride = int((self.T * self.spec.max_bits + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=self.state.device)
        self.ranked = None
        self.rank_stride = 0

    def enable_export(self):
        """Register a [B, K + 1] rank export for the steps of this session; returns it."""
        torch = _torch()
        self.rank_stride = self.spec.K + 1
        self.ranked = torch.full((self.B, self.rank_stride), -1, dtype=torch.int32, device=self.state.device)
        return self.ranked

    def step(self, logits) -> None:
        if self.t >= self.T:
            raise ConfigurationError("all tokens already decoded")
        t = self.t
        _check_logits(self.ctx, self.B, logits)
        L = _lib.lib()
        if self.ranked is not None:
            self.ctx.check(L.ns_set_rank_export(self.ctx._h, _ptr(self.ranked), self.rank_stride), "ns_set_rank_export")
        rc = self.spec.entry("decode_step")(
            *self.spec.head(self.ctx, logits, self.B), _ptr(self.tok[t]), _ptr(self.act[t]), _ptr(self.state),
            _ptr(self.out_bits), self.out_stride, self.ctx._banned, self.ctx._nbanned, _ptr(self.trace), 0,
            _stream_handle())
        if self.ranked is not None:
            L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, f"ns_{self.spec.mode}_decode_step")
        self.t += 1

    def step_static(self, logits, **kw):
        raise ConfigurationError("the baseline coders' table-driven decode is BaselineDecodeStreamsSession")

    def bits(self) -> List[List[int]]:
        f = _state_fields(self.state)
        bad = np.nonzero(f["flags"] & _lib.NS_ST_ERR_RANGE)[0]
        if bad.size:
            raise ArithmeticRangeError(f"streams {bad.tolist()[:8]}: a row the {self.spec.mode} coder cannot code")
        bad = np.nonzero(f["flags"] & _lib.NS_ST_ERR_DIVERGE)[0]
        if bad.size:
            raise DecodeDivergenceError(f"streams {bad.tolist()[:8]}: received token outside the {self.spec.mode} code")
        return _bit_rows_to_lists(self.out_bits, f["bit_pos"])


class BaselineStreamingDecodeSession(StreamingDecodeSession):
    """:class:`StreamingDecodeSession` of a baseline coder: the host supplies each step's tokens (the text decoders'
    BPE repairs edit the token lists mid-stream); a diverged stream exports its K ranked leaders (Huffman) or every
    bin's token in bin order (bins)."""

    def __init__(self, ctx: CoderContext, B: int, max_tokens: int, *, mode: str, block_size: int, table=None):
        self.spec = BaselineSpec(ctx, mode, block_size, table)
        super().__init__(ctx, B, max_tokens)
        torch = _torch()
        self.P = self.spec.max_bits
        self.out_stride = int((max(1, max_tokens) * self.P + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=self.dev)
        self.rank_stride = self.spec.K + 1
        self.ranked = torch.full((self.B, self.rank_stride), -1, dtype=torch.int32, device=self.dev)

    def step(self, logits, tokens: Sequence[int], active: Sequence[bool]) -> None:  # type: ignore[override]
        torch = _torch()
        _check_logits(self.ctx, self.B, logits)
        f = _state_fields(self.state)
        self._grow(int(f["bit_pos"].max(initial=0)) + 2 * self.P)
        tok = torch.tensor(np.asarray(tokens, dtype=np.int32), device=self.dev)
        act = torch.tensor(np.asarray(active, dtype=np.uint8), device=self.dev)
        L = _lib.lib()
        self.ctx.check(L.ns_set_rank_export(self.ctx._h, _ptr(self.ranked), self.rank_stride), "ns_set_rank_export")
        rc = self.spec.entry("decode_step")(
            *self.spec.head(self.ctx, logits, self.B), _ptr(tok), _ptr(act), _ptr(self.state), _ptr(self.out_bits),
            self.out_stride, self.ctx._banned, self.ctx._nbanned, ctypes.c_void_p(0), 0, _stream_handle())
        L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, f"ns_{self.spec.mode}_decode_step")

    def range_errors(self) -> List[int]:
        f = _state_fields(self.state)["flags"]
        return np.nonzero(f & _lib.NS_ST_ERR_RANGE)[0].tolist()


class BaselineDecodeStreamsSession(DecodeStreamsSession):
    """:class:`DecodeStreamsSession` of a baseline coder (``ns_huffman_decode_step_streams`` /
    ``ns_bins_decode_step_streams``): every slot decodes the token at its own ``ntokens`` from its device token
    row, so the slot loop needs no host read and one captured step serves every step."""

    def __init__(self, ctx: CoderContext, S: int, *, max_tokens: int, mode: str, block_size: int, table=None,
                 rank_export: bool = True):
        torch = _torch()
        self.spec = BaselineSpec(ctx, mode, block_size, table)
        self.ctx, self.B = ctx, int(S)
        if self.B < 1 or self.B > ctx.max_batch:
            raise ConfigurationError(f"batch {self.B} outside [1, {ctx.max_batch}]")
        dev = torch.device("cuda", ctx.device)
        self.T = max(1, int(max_tokens))
        self.k_max, self.P = self.spec.K, self.spec.max_bits
        self.tokmat = torch.zeros((self.B, self.T), dtype=torch.int32, device=dev)
        self.nlen = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.B, self.T), dtype=torch.int64, device=dev)
        self.out_token = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.out_stride = int((self.T * self.P + 7) // 8 + 8)
        self.out_bits = torch.zeros((self.B, self.out_stride), dtype=torch.uint8, device=dev)
        self.qtable = None
        self.state = _state_tensor(self.B, dev)
        self.rank_stride = self.spec.K + 1
        self.ranked = torch.full((self.B, self.rank_stride), -1, dtype=torch.int32, device=dev) if rank_export \
            else None
        self.trace = None
        self.steps = 0

    def step(self, logits):  # type: ignore[override]
        _check_logits(self.ctx, self.B, logits)
        L = _lib.lib()
        if self.ranked is not None:
            self.ctx.check(L.ns_set_rank_export(self.ctx._h, _ptr(self.ranked), self.rank_stride), "ns_set_rank_export")
        rc = self.spec.entry("decode_step_streams")(
            *self.spec.head(self.ctx, logits, self.B), _ptr(self.tokmat), self.T, _ptr(self.nlen), _ptr(self.state),
            _ptr(self.out_bits), self.out_stride, _ptr(self.counts), self.T, _ptr(self.out_token), self.ctx._banned,
            self.ctx._nbanned, _ptr(self.trace), 0, _stream_handle())
        if self.ranked is not None:
            L.ns_set_rank_export(self.ctx._h, ctypes.c_void_p(0), 0)
        self.ctx.check(rc, f"ns_{self.spec.mode}_decode_step_streams")
        self.steps += 1
        return self.out_token

    def load_slots(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], quality=None) -> None:
        """Start new streams in ``slots``: their tokens and count, a zeroed state, output bytes and counts."""
        torch = _torch()
        n = len(slots)
        if n == 0:
            return
        if len(token_lists) != n:
            raise ConfigurationError("load_slots: one token list per slot")
        tok = np.zeros((n, self.T), dtype=np.int32)
        nl = np.zeros(n, dtype=np.int32)
        for i, tl in enumerate(token_lists):
            k = len(tl)
            if k > self.T:
                raise ConfigurationError("stream longer than the session was sized for")
            tok[i, :k] = np.asarray(tl, dtype=np.int32)
            nl[i] = k
        dev = self.state.device
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=dev)
        self.tokmat[idx] = torch.from_numpy(tok).to(dev)
        self.nlen[idx] = torch.from_numpy(nl).to(dev)
        self.state[idx] = 0
        self.out_bits[idx] = 0
        self.counts[idx] = 0


def baseline_encode_batch(ctx: CoderContext, payload_bits: Sequence[Sequence[int]], logits_fn, *, mode: str,
                          block_size: int, max_steps: int = 1 << 20, check_every: int = 32, finish_sent: bool = False,
                          return_stats: bool = False, table=None):
    """:func:`encode_batch` for a baseline coder: steps until every stream has consumed its payload (and, with
    ``finish_sent``, ended its sentence); ``logits_fn(step, last_tokens)`` gives each step's ``[B, ld]`` logits."""
    sess = BaselineEncodeSession(ctx, payload_bits, mode=mode, block_size=block_size, stats=return_stats, table=table)
    last = sess.out_token
    for t in range(max_steps):
        if t % check_every == 0:
            if sess.all_done():
                break
            sess.ensure_history(check_every)
        last = sess.step(logits_fn(t, last), finish_sent=finish_sent)
    else:
        raise ConfigurationError("encode did not finish within max_steps")
    if return_stats:
        return sess.tokens(), sess.stats()
    return sess.tokens()


def baseline_decode_batch(ctx: CoderContext, token_lists: Sequence[Sequence[int]], logits_fn, *, mode: str,
                          block_size: int, table=None) -> List[List[int]]:
    sess = BaselineDecodeSession(ctx, token_lists, mode=mode, block_size=block_size, table=table)
    for t in range(sess.T):
        sess.step(logits_fn(t, sess.tok[t]))
    return sess.bits()
