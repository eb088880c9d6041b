"""Batched GPT-2 forward with a KV cache, writing logits straight into the coder's layout.

This is the L1 "LM runtime" of SURVEY.md §1 rebuilt for batch B (PyTorch-ROCm holds the weights; in the fp16 GPU
configuration every GEMM and attention of the forward runs on the library's own MFMA kernels over a paged KV cache,
see below).  It reproduces the reference's forward semantics (``code_base/arithmetic.py:12-48,115-122``):

* the first call runs the whole context with default positions ``0..T-1``;
* every later call feeds ONE token per stream with ``position_ids = cache_len % n_positions``
  (``_position_ids_for_cache``, ``:44-48``) and attends to the whole cache: the reference never truncates
  it (``limit_past`` slices head_dim, a no-op, ``code_base/utils.py:19-30``).

In fp16 on the GPU (the product configuration) every forward runs on hand-written HIP kernels whose per-stream
results do not depend on the batch size (``include/nsg_lm.h``: MFMA GEMMs with the bias / gelu / residual
epilogues fused, layer norms, embedding; ``include/nsg_attn.h``: the decode step's KV append fused with a
fixed-split online-softmax attention over each stream's pages (``lm/kvpages.py``), HBM-bound on the cache, and a
causal MFMA flash attention for whole sequences): the decode steps, the shared-context prefill, the guard's scoring
forward and the ``max_context`` window forward.  A cover encoded in a batch of B streams decodes to the same logits
alone, and a text scores the same alone or in a batch.  fp32 compute and the CPU keep PyTorch (``addmm`` +
``scaled_dot_product_attention`` over a dense ``k_cache``/``v_cache``) as the forward's reference configuration
(tests pin the two against each other and against Hugging Face).

Logits are produced as ``h @ wte^T`` into a ``[B, ld]`` buffer with ``ld = row_stride(V)`` (zero weight
columns beyond V), so the coder reads 16-byte-aligned rows without a copy.  Weights are taken from a
Hugging Face ``GPT2LMHeadModel`` (pretrained when available offline, random-init otherwise).
"""

from __future__ import annotations

import math
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from ..coder import row_stride


@dataclass
class GPT2Shape:
    n_layer: int
    n_head: int
    n_embd: int
    vocab: int
    n_positions: int
    eps: float


class BatchedGPT2:
    """GPT-2 decoder for B streams: one token per stream and step, each stream at its own cache length on the
    native path (``kv``, the page table the slot schedulers drive), all at ``L`` on the PyTorch path.

    ``compute_dtype`` is the weight/activation dtype (fp16 on the GPU by default); ``logits_dtype`` is what
    the coder reads (``torch.float32`` or ``torch.float16``)."""

    def __init__(self, hf_model, *, device=None, compute_dtype=None, logits_dtype=torch.float32, kv_dtype="fp16",
                 logit_scale: float = 1.0):
        cfg = hf_model.config
        self.shape = GPT2Shape(cfg.n_layer, cfg.n_head, cfg.n_embd, cfg.vocab_size, cfg.n_positions,
                               cfg.layer_norm_epsilon)
        self.device = _normalise_device(torch.device(device) if device is not None else next(hf_model.parameters()).device)
        if compute_dtype is None:
            compute_dtype = torch.float16 if self.device.type == "cuda" else torch.float32
        self.dtype = compute_dtype
        self.logits_dtype = logits_dtype
        self.ld = row_stride(self.shape.vocab, "f16" if logits_dtype == torch.float16 else "f32")
        sd = {k: v.detach() for k, v in hf_model.state_dict().items()}
        dev, dt = self.device, self.dtype

        def w(name):
            return sd[name].to(device=dev, dtype=dt).contiguous()

        pre = "transformer."
        self.wte = w(pre + "wte.weight")
        self.wpe = w(pre + "wpe.weight")
        self.layers = []
        for i in range(self.shape.n_layer):
            p = f"{pre}h.{i}."
            self.layers.append({
                "ln1_w": w(p + "ln_1.weight"), "ln1_b": w(p + "ln_1.bias"),
                "qkv_w": w(p + "attn.c_attn.weight"), "qkv_b": w(p + "attn.c_attn.bias"),
                "o_w": w(p + "attn.c_proj.weight"), "o_b": w(p + "attn.c_proj.bias"),
                "ln2_w": w(p + "ln_2.weight"), "ln2_b": w(p + "ln_2.bias"),
                "fc_w": w(p + "mlp.c_fc.weight"), "fc_b": w(p + "mlp.c_fc.bias"),
                "pr_w": w(p + "mlp.c_proj.weight"), "pr_b": w(p + "mlp.c_proj.bias"),
            })
        self.lnf_w = w(pre + "ln_f.weight")
        self.lnf_b = w(pre + "ln_f.bias")
        # lm_head = wte^T padded to ld columns (zeros beyond V): logits land in the coder's row layout
        # logit_scale != 1 (synthetic "trained-entropy" rows, bench / tests only): the head alone is scaled, so a
        # random-init model's near-uniform rows (~15 bits of entropy) peak like a trained LM's (a few bits)
        head = torch.zeros((self.shape.n_embd, self.ld), device=dev, dtype=dt)
        head[:, : self.shape.vocab] = self.wte.t() if logit_scale == 1.0 else (self.wte.float().t() * float(logit_scale)).to(dt)
        self.head = head
        self.B = 0
        self.L = 0
        self.T0 = 0  # positions held once in the shared prefix cache (kp, vp) instead of per stream
        self.position_cap = None  # optional cap on the initial per-stream cache length (the cache still grows)
        # attention window (opt-in, 0 = the reference's unbounded cache): decode steps attend to the last `window`
        # positions only -- a sliding-window approximation bounding the per-step KV traffic (native path only)
        self.window = 0
        self.kp = self.vp = None
        self.k_cache = self.v_cache = None  # dense [layer, B, H, rows, D] cache of the PyTorch path only
        # Decode steps in fp16 on the GPU run entirely on the batch-invariant HIP kernels (include/nsg_lm.h and
        # the fixed-split attention of include/nsg_attn.h; fail loudly if the library is missing): a stream's
        # logits are bit-identical whatever the batch it runs in, so a cover encoded among B streams decodes
        # alone.  Weights are kept transposed ([N, K], K contiguous).  fp32 compute and the CPU keep the PyTorch
        # path (SDPA), the forward's reference configuration in the tests.
        self.native = self.device.type == "cuda" and self.dtype == torch.float16
        # KV cache element type: "fp16" (the reference configuration) or "fp8" (OCP e4m3fn, opt-in: half the
        # bytes the HBM-bound decode attention reads; logits differ at the fp8 quantisation level, the same for
        # encoder and decoder, batch-invariant)
        if kv_dtype not in ("fp16", "fp8"):
            raise ValueError("kv_dtype must be 'fp16' or 'fp8'")
        if kv_dtype == "fp8" and not self.native:
            raise ValueError("an fp8 KV cache needs the native fp16 decode step on the GPU")
        self.kv_dtype = kv_dtype
        self.kv_torch_dtype = torch.uint8 if kv_dtype == "fp8" else self.dtype
        self._static_logits = None
        # native path: the paged KV cache (lm/kvpages.py) -- a pool of 32-position pages kept across calls, and the
        # current call's page table + per-stream lengths
        self.pool = None
        self.kv = None
        self.kv_segment_pages = None  # pages per pool segment (None: from the first call's batch)
        self.first_logits = None  # [1, ld] logits of the shared context (a refilled slot's first coder step)
        # prefill_contexts: packed context rows per group of whole sequences.  The workspace of a packed row is
        # about 10 C fp16 values (h, a, o: 3 C, qkv: 3 C, c_fc: 4 C; 15 KB at C = 768), so 65,536 rows is about 1 GB
        # for GPT-2-small -- derived from those sizes, not measured
        self.prefill_row_budget = 65536
        self.last_prefill = None  # {"rows", "groups", "shared"} of the last prefill_contexts call
        self.share_contexts = True  # equal contexts of a call share their KV pages (off: A/B runs and tests)
        # different contexts of a call share the pages of a common prefix, in 64-row blocks (lm/kvpages.py); in
        # effect only with share_contexts on and fp16 pages (``prefix_sharing``)
        self.share_prefixes = True
        # optional per-stream done flags read by the decode attention (int32 tensor view [B], bit 0 = finished, e.g.
        # the coder state's flags word): finished streams skip their cache reads; their logits are never used again
        self.done_flags = None
        # optional per-stream stop positions (int32 [B]): a stream whose cache length reached its stop skips its
        # attention (decode: the position after which its logits are no longer read)
        self.stop_len = None
        if self.native:
            from .. import _lib

            _lib.lib()  # a missing library fails here, not at the first step
            self._kv_format = _lib.NS_KV_FP8 if kv_dtype == "fp8" else _lib.NS_KV_FP16
            if self.shape.n_embd // self.shape.n_head != 64:
                raise ValueError("the HIP decode attention needs head_dim 64 (GPT-2 small/medium/large)")
            for lw in self.layers:
                for name in ("qkv", "o", "fc", "pr"):
                    lw[name + "_wt"] = lw[name + "_w"].t().contiguous()
            self.head_t = self.head.t().contiguous()  # [ld, C]: wte rows, zero rows beyond V
            self._nb = None

    # ------------------------------------------------------------------
    def kv_bytes_per_position(self, B: int) -> int:
        s = self.shape
        return 2 * s.n_layer * B * s.n_embd * torch.tensor([], dtype=self.kv_torch_dtype).element_size()

    def headroom_bytes(self, B: int) -> int:
        """Device memory kept free beside the KV cache for what is allocated after it: the logit
        rows of the step (fixed graph buffer, a coder-side copy, the decoder's), the wide coder path's scratch
        (two 8-byte key arrays per id), the activation buffers of the native step and the guard's scoring chunk,
        plus 2 GiB for the runtime and the allocator's rounding."""
        s = self.shape
        per_stream = self.ld * 4 * 3 + s.vocab * 16 + 16 * s.n_embd * 2
        return (2 << 30) + int(B) * per_stream

    def fit_positions(self, B: int, want: int, reserve: float = 0.05, count_cached: bool = True) -> int:
        """Largest cache length <= ``want`` that fits the device's free memory, minus :meth:`headroom_bytes` and
        a ``reserve`` fraction.  The reference's cache is unbounded; at B = 4096 a 1 KiB payload needs ~1.1k
        positions (170 GB for GPT-2-small fp16), so the budget is sized from what is free, not guessed."""
        if self.position_cap is not None:
            want = min(int(want), int(self.position_cap))
        if self.device.type != "cuda":
            return int(want)
        # the previous cache is dropped first; memory PyTorch's caching allocator holds but no tensor uses (e.g.
        # that cache, or the pre-touched one bench.py hands back) counts as free: reusing those segments keeps
        # the pages warm (releasing them and allocating afresh measured a much slower first pass over the new
        # cache).  When a small tensor carved out of a freed block makes the request not fit the hole (seen as a
        # 120 GiB OOM between two encodes of different batch sizes), _allocate_fitted releases the idle segments
        # and sizes the cache again from what the device then reports free (count_cached=False).
        self.k_cache = self.v_cache = None
        free, _ = torch.cuda.mem_get_info(self.device)
        if count_cached:
            free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        budget = int(free * (1.0 - reserve)) - self.headroom_bytes(B)
        return max(1, min(int(want), budget // self.kv_bytes_per_position(B)))

    def _native_buffers(self, B: int):
        """Activation buffers of the native decode step (fixed addresses: a captured graph replays them)."""
        if self._nb is None or self._nb["B"] != B:
            C, dev, dt = self.shape.n_embd, self.device, self.dtype
            self._nb = {"B": B, "h": torch.empty((B, C), device=dev, dtype=dt),
                        "a": torch.empty((B, C), device=dev, dtype=dt),
                        "qkv": torch.empty((B, 3 * C), device=dev, dtype=dt),
                        "o": torch.empty((B, C), device=dev, dtype=dt),
                        "f": torch.empty((B, 4 * C), device=dev, dtype=dt)}
        return self._nb

    def _cache_shape(self, B: int, rows: int):
        s = self.shape
        return (s.n_layer, B, s.n_head, rows, s.n_embd // s.n_head)

    def _allocate_fitted(self, B: int, base: int, want: int, T0: int = 0) -> None:
        """allocate(B, base + fit_positions(B, want)), falling back to a fresh budget after releasing PyTorch's
        idle segments when the cached ones are too fragmented for the request."""
        try:
            self.allocate(B, base + self.fit_positions(B, want), T0=T0)
        except torch.OutOfMemoryError:
            self.k_cache = self.v_cache = None
            torch.cuda.empty_cache()
            self.allocate(B, base + self.fit_positions(B, want, count_cached=False), T0=T0)

    def allocate(self, B: int, max_len: int, T0: int = 0) -> None:
        """Dense per-stream KV cache of the PyTorch path (``k_cache``/``v_cache``, plain [layer, B, H, rows, D]
        rows) for absolute positions [T0, max_len).  The native path pages instead (:meth:`begin_slots`)."""
        self.k_cache = self.v_cache = None
        shp = self._cache_shape(B, max_len - T0)
        # uninitialised: attention only ever reads positions < L + 1, all written before they are read
        self.k_cache = torch.empty(shp, device=self.device, dtype=self.kv_torch_dtype)
        self.v_cache = torch.empty(shp, device=self.device, dtype=self.kv_torch_dtype)
        self.B, self.L, self.max_len, self.T0 = B, 0, max_len, T0
        if T0 == 0:
            self.kp = self.vp = None

    def grow(self, extra: int) -> None:
        """Enlarge the dense KV cache of the PyTorch path (fp32 / CPU, the forward's reference configuration) by
        ``extra`` positions, copying the filled part.  The copy holds the old and the new cache at once, so the
        WHOLE new cache must fit beside the old one (the native path pages instead: no copy)."""
        from ..exceptions import KVCapacityError

        new_len = self.max_len + int(extra)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
            fit = (int(free * 0.9) - self.headroom_bytes(self.B)) // self.kv_bytes_per_position(self.B) + self.T0
            new_len = min(new_len, fit)
            if new_len <= self.L:
                raise KVCapacityError(f"KV cache full at {self.L} positions for B={self.B}: no device memory to grow")
        T0, n = self.T0, self.L - self.T0  # stream rows filled so far
        shp = self._cache_shape(self.B, new_len - T0)
        k = torch.empty(shp, device=self.device, dtype=self.k_cache.dtype)
        v = torch.empty(shp, device=self.device, dtype=self.v_cache.dtype)
        k[:, :, :, :n] = self.k_cache[:, :, :, :n]
        v[:, :, :, :n] = self.v_cache[:, :, :, :n]
        self.k_cache, self.v_cache, self.max_len = k, v, new_len

    def _ln(self, x, wgt, b):
        return F.layer_norm(x, (self.shape.n_embd,), wgt, b, self.shape.eps)

    def _block(self, i, h, positions_new: int, causal: bool):
        s = self.shape
        lw = self.layers[i]
        B, T, C = h.shape
        H, D = s.n_head, C // s.n_head
        a = self._ln(h, lw["ln1_w"], lw["ln1_b"])
        qkv = torch.addmm(lw["qkv_b"], a.reshape(B * T, C), lw["qkv_w"]).view(B, T, 3, H, D)
        q = qkv[:, :, 0].transpose(1, 2)
        k = qkv[:, :, 1].transpose(1, 2)
        v = qkv[:, :, 2].transpose(1, 2)
        L0 = self.L
        self.k_cache[i, :B, :, L0:L0 + T] = k
        self.v_cache[i, :B, :, L0:L0 + T] = v
        kk = self.k_cache[i, :B, :, : L0 + T]
        vv = self.v_cache[i, :B, :, : L0 + T]
        if causal:
            o = F.scaled_dot_product_attention(q, kk, vv, is_causal=True)
        else:
            o = F.scaled_dot_product_attention(q, kk, vv)
        o = o.transpose(1, 2).reshape(B * T, C)
        h = h + torch.addmm(lw["o_b"], o, lw["o_w"]).view(B, T, C)
        m = self._ln(h, lw["ln2_w"], lw["ln2_b"])
        f = F.gelu(torch.addmm(lw["fc_b"], m.reshape(B * T, C), lw["fc_w"]), approximate="tanh")
        h = h + torch.addmm(lw["pr_b"], f, lw["pr_w"]).view(B, T, C)
        return h

    def _logits(self, h_last):
        hf = self._ln(h_last, self.lnf_w, self.lnf_b)
        out = hf @ self.head
        return out if out.dtype == self.logits_dtype else out.to(self.logits_dtype)

    def _quantize_fp8(self, t: torch.Tensor) -> torch.Tensor:
        from .. import _lib
        from ..coder import _stream_handle

        src = t.contiguous()
        out = torch.empty(src.shape, device=src.device, dtype=torch.uint8)
        if src.numel() % 4:
            raise ValueError("fp8 quantisation needs a multiple of 4 elements")
        _check(_lib.lib().ns_quantize_fp8(src.data_ptr(), out.data_ptr(), src.numel(), _stream_handle()),
               "ns_quantize_fp8")
        return out

    @torch.no_grad()
    def prefill(self, context: Sequence[int], B: int, max_new: int) -> torch.Tensor:
        """Run the shared context once (reference: first call, default positions) and broadcast its cache
        to B streams.  Returns the ``[B, ld]`` logits for the next token."""
        ctx = [int(t) for t in list(context)[-1022:]]  # code_base/arithmetic.py:90
        T = len(ctx)
        if T < 1:
            raise ValueError("context must contain at least one token")
        if min(ctx) < 0 or max(ctx) >= self.shape.vocab:  # host check: never gather out of the table
            raise ValueError(f"context token ids must lie in [0, {self.shape.vocab})")
        ids = torch.tensor([ctx], device=self.device, dtype=torch.long)
        if self.native:
            # the context runs once on the native sequence kernels (MFMA GEMMs + causal MFMA attention, no PyTorch
            # attention or BLAS), and its K/V -- the same for every stream -- are kept ONCE (kp/vp), read by every
            # stream's attention (ns_decode_attention_prefix): B-fold less prefix traffic and memory, identical bits
            s = self.shape
            H, D, C = s.n_head, s.n_embd // s.n_head, s.n_embd
            kp = torch.empty((s.n_layer, 1, H, T, D), device=self.device, dtype=self.dtype)
            vp = torch.empty_like(kp)

            def keep_kv(i, qkv):
                kp[i, 0] = qkv[:, C:2 * C].view(T, H, D).transpose(0, 1)
                vp[i, 0] = qkv[:, 2 * C:].view(T, H, D).transpose(0, 1)

            self.kv = None
            hs = self._seq_native(ids, kv_hook=keep_kv)
            lg = self._head_native(hs[T - 1:T])
            if self.kv_dtype == "fp8":  # the context rows get the same conversion as the decode-time appends
                kp, vp = self._quantize_fp8(kp), self._quantize_fp8(vp)
            self.kp, self.vp = kp, vp
            self.first_logits = lg
            self.begin_slots(B, T, max_new)
            return lg.repeat(B, 1)  # always a copy: slot refills write first_logits into these rows
        else:
            pos = torch.arange(T, device=self.device) % self.shape.n_positions
            h = self.wte[ids] + self.wpe[pos][None]
            self._allocate_fitted(B, 0, T + max_new)
            if self.max_len < T + 1:
                raise RuntimeError(f"no device memory for a {T + 1}-position KV cache at B={B}")
            # run the context for one stream, then copy its cache to every stream
            saveB = self.B
            self.B = 1
            for i in range(self.shape.n_layer):
                h = self._block(i, h, T, causal=True)
            self.B = saveB
            for i in range(self.shape.n_layer):
                self.k_cache[i, 1:B, :, :T] = self.k_cache[i, 0:1, :, :T]
                self.v_cache[i, 1:B, :, :T] = self.v_cache[i, 0:1, :, :T]
        self.L = T
        lg = self._logits(h[:, -1])
        return lg.expand(B, -1).contiguous()

    def _seq_native(self, ids: torch.Tensor, kv_hook=None) -> torch.Tensor:
        """Causal forward of B whole sequences ``[B, T]`` (positions 0..T-1, no cache) on the native kernels:
        embedding + ln_1, then per layer the c_attn GEMM, the causal MFMA attention (``ns_seq_attention``), c_proj
        with the residual in its epilogue, ln_2, c_fc with gelu_new, c_proj + residual.  Returns the residual
        stream ``[B*T, C]`` before ln_f.  Every row's result depends on its own sequence only (the GEMMs' and the
        attention's batch invariance), so a text scores the same alone or in a batch.  ``kv_hook(layer, qkv)``
        sees each layer's ``[B*T, 3C]`` c_attn output (the prefill keeps the context's K/V)."""
        from .. import _lib
        from ..coder import _stream_handle

        s = self.shape
        B, T = ids.shape
        C, H = s.n_embd, s.n_head
        D = C // H
        L = _lib.lib()
        st = _stream_handle()
        tok = ids.to(device=self.device, dtype=torch.int32).reshape(B * T).contiguous()

        def embed(h, a, lw0, eps):
            _check(L.ns_lm_embed_seq_ln(tok.data_ptr(), self.wte.data_ptr(), self.wpe.data_ptr(), s.vocab,
                                        s.n_positions, T, h.data_ptr(), C, lw0["ln1_w"].data_ptr(),
                                        lw0["ln1_b"].data_ptr(), a.data_ptr(), C, B * T, C, eps, st),
                   "ns_lm_embed_seq_ln")

        def attention(i, qkv, o):
            if kv_hook is not None:
                kv_hook(i, qkv)
            _check(L.ns_seq_attention(qkv.data_ptr(), qkv.stride(0), o.data_ptr(), o.stride(0), B, T, H, D,
                                      1.0 / math.sqrt(D), st), "ns_seq_attention")

        return self._rows_native(B * T, embed, attention)

    def _rows_native(self, M: int, embed, attention) -> torch.Tensor:
        """The layer stack of :meth:`_seq_native` over ``M`` token rows: ``embed(h, a, layer0, eps)`` fills the
        residual stream and its ln_1, ``attention(layer, qkv, o)`` turns a layer's ``[M, 3C]`` c_attn output into the
        ``[M, C]`` attention rows (how the rows group into sequences is the caller's: equal lengths, or ragged)."""
        from .. import _lib
        from ..coder import _stream_handle

        s = self.shape
        C = s.n_embd
        L = _lib.lib()
        st = _stream_handle()
        dev, dt = self.device, self.dtype
        h = torch.empty((M, C), device=dev, dtype=dt)
        a = torch.empty_like(h)
        o = torch.empty_like(h)
        qkv = torch.empty((M, 3 * C), device=dev, dtype=dt)
        f = torch.empty((M, 4 * C), device=dev, dtype=dt)
        eps = float(s.eps)

        def gemm(x, wt, bias, y, epi, N, K):
            _check(L.ns_lm_gemm(x.data_ptr(), x.stride(0), wt.data_ptr(), wt.stride(0), bias.data_ptr(),
                                y.data_ptr(), y.stride(0), M, N, K, epi, st), "ns_lm_gemm")

        def ln(x, w, b, y):
            _check(L.ns_lm_layernorm(x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y.data_ptr(), C, M, C, eps, st),
                   "ns_lm_layernorm")

        embed(h, a, self.layers[0], eps)
        for i, lw in enumerate(self.layers):
            if i > 0:
                ln(h, lw["ln1_w"], lw["ln1_b"], a)
            gemm(a, lw["qkv_wt"], lw["qkv_b"], qkv, _lib.NS_LM_EPI_STORE, 3 * C, C)
            attention(i, qkv, o)
            gemm(o, lw["o_wt"], lw["o_b"], h, _lib.NS_LM_EPI_RESIDUAL, C, C)
            ln(h, lw["ln2_w"], lw["ln2_b"], a)
            gemm(a, lw["fc_wt"], lw["fc_b"], f, _lib.NS_LM_EPI_GELU, 4 * C, C)
            gemm(f, lw["pr_wt"], lw["pr_b"], h, _lib.NS_LM_EPI_RESIDUAL, C, 4 * C)
        return h

    # ------------------------------------------------------------------ one context per stream (native path)
    @property
    def prefix_sharing(self) -> bool:
        """Whether contexts share the pages of a common prefix: ``share_prefixes`` and ``share_contexts`` on the native
        path with fp16 pages.  fp8 pages hold converted values while a whole prefill attends over the fp16 rows: a
        prefill continued from them could not give the same bits, so it is not done."""
        from .. import _lib

        return bool(self.native and self.share_prefixes and self.share_contexts and
                    self._kv_format == _lib.NS_KV_FP16)

    @torch.no_grad()
    def prefill_contexts(self, contexts: Sequence[Sequence[int]], slots, shared=None, chains=None) -> torch.Tensor:
        """Run one context PER stream and leave each in its stream's own KV pages: ``contexts[i]`` (trimmed to its
        last 1,022 ids as :meth:`prefill` trims) becomes positions ``0..T_i-1`` of slot ``slots[i]`` of a call begun
        with ``begin_slots(B, 0, ...)`` (pages for those positions are mapped here unless the caller already has).
        The contexts are packed back to back and run as ragged sequences: embedding + ln_1 at each row's own
        position, the layer GEMMs over the packed rows, ``ns_seq_attention_ragged`` writing every layer's K/V into
        the pages.  Sets ``lens[slot] = T_i`` (device and host mirror) and returns the ``[n, ld]`` logits after each
        context's last token.  Row ``i`` equals ``prefill(contexts[i], 1, ...)``'s logits bit for bit, and the decode
        steps that follow read the same K/V values in the same order as over a shared prefix: a message's tokens do
        not depend on how its context reached the cache.  Whole sequences are run in groups of at most
        ``prefill_row_budget`` packed rows (a longer single context runs alone): grouping bounds the workspace,
        never the bits.

        Equal contexts share pages (``share_contexts``; ``shared``: one flag per context, from a scheduler that knows
        the whole call's multiplicities -- default: a context shares when a live entry of ``kv.entries`` holds it or
        another context of this call equals it).  A sharing context is run once, into its entry's own pages through a
        small table of those pages, while any slot holds the entry; every holder's table row starts with the entry's
        full pages, the context's last partial page is copied into the holder's first own page (``ns_kv_copy_rows``:
        the holder appends into it) and its logits row is the entry's.  The stored bytes are the ones a private
        prefill stores and the decode step reads by address, so the bits do not change.  ``last_prefill`` has the
        ``rows`` actually run, the ``groups`` they ran in and ``shared``, the slots served from an entry.

        Different contexts share the pages of a common prefix (``prefix_sharing``; ``chains``: one chain of
        :func:`kvpages.plan_prefixes` per context, from a scheduler that planned the whole call -- default: planned
        over this call's contexts, and none when ``shared`` is given without it).  The prefix entries that are new run
        first, level by level, parents before children, each over its own rows only; then every context's remaining
        rows -- an equal-context entry's, a private suffix's or a singleton's -- at positions ``past + index`` through
        ``ns_seq_attention_ragged_past``, which takes the key blocks below ``past`` from the chain's pages.  A split at
        a multiple of 64 changes no bit (the kernel's contract), the other kernels are row-wise, and a context's
        logits row is its last new row's: row ``i`` still equals ``prefill(contexts[i], 1, ...)``.  A run in which
        every ``past`` is 0 calls ``ns_seq_attention_ragged`` as before.  When a prefix was shared ``last_prefill``
        also has ``prefix_rows_saved``, the rows not run for it, and ``prefix_entries``, the prefix entries run."""
        if not self.native:
            raise RuntimeError("prefill_contexts needs the native HIP path (fp16 on the GPU)")
        kv = self.kv
        if kv is None or kv.T0 != 0:
            raise RuntimeError("prefill_contexts needs a call begun with begin_slots(B, 0, ...)")
        ctxs = [[int(t) for t in list(c)[-1022:]] for c in contexts]  # code_base/arithmetic.py:90
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        n = len(ctxs)
        if n == 0 or slots.size != n:
            raise ValueError("one slot per context, at least one context")
        if np.unique(slots).size != n or slots.min() < 0 or slots.max() >= kv.B:
            raise ValueError(f"slots must be distinct rows of the {kv.B}-slot table")
        for c in ctxs:
            if len(c) < 1:
                raise ValueError("context must contain at least one token")
            if min(c) < 0 or max(c) >= self.shape.vocab:  # host check: never gather out of the table
                raise ValueError(f"context token ids must lie in [0, {self.shape.vocab})")
        from ..exceptions import KVCapacityError

        from .kvpages import plan_prefixes

        lens = np.asarray([len(c) for c in ctxs], dtype=np.int64)
        # only slots that can take a hold (no page mapped yet) or have one are compared: a context whose twin keeps
        # private pages stays a singleton, it does not open an entry for itself alone
        el = [i for i, s in enumerate(slots.tolist())
              if kv.nch[s] == 0 or kv.slot_entry[s] is not None or kv.slot_prefix[s] is not None]
        if chains is None:
            chains = [()] * n
            if shared is None and self.prefix_sharing and len(el) > 1:
                for i, ch in zip(el, plan_prefixes([ctxs[i] for i in el])):
                    chains[i] = ch
        elif len(chains) != n:
            raise ValueError("one prefix chain per context")
        elif any(chains) and not self.prefix_sharing:
            raise ValueError("prefix chains need prefix_sharing (fp16 pages, share_contexts and share_prefixes)")
        if shared is None:  # a context shares when a live entry holds it or another context of this call equals it
            from .kvpages import sharing_keys

            keys = [None] * n
            if self.share_contexts and el:
                for i, k in zip(el, sharing_keys([ctxs[i] for i in el], kv.entries)):
                    keys[i] = k
            sh = np.asarray([k is not None for k in keys], dtype=bool)
        else:
            sh = np.asarray(shared, dtype=bool).reshape(-1)
            if sh.size != n:
                raise ValueError("one shared flag per context")
            keys = [tuple(c) if f else None for c, f in zip(ctxs, sh)]
        # holders: their table rows start with the chain's and the entry's full pages (a scheduler may have mapped them)
        # (a call of unrelated contexts has nothing held: the loops below run over the holders only)
        held = [i for i, s in enumerate(slots.tolist()) if sh[i] or chains[i] or kv.slot_prefix[s] is not None]
        todo = [i for i in held if kv.slot_entry[slots[i]] is None and kv.slot_prefix[slots[i]] is None]
        if todo and kv.hold(slots[todo], [keys[i] for i in todo], lens[todo], [chains[i] for i in todo]).size:
            kv.release(slots[todo])
            raise KVCapacityError("no device memory for a shared context's KV pages")
        past = np.zeros(n, dtype=np.int64)  # rows a slot's own run skips: its private suffix starts there
        for i in held:
            e, p = kv.slot_entry[slots[i]], kv.slot_prefix[slots[i]]
            if sh[i]:
                if e is None or e.key != keys[i]:
                    raise RuntimeError("prefill_contexts: the slot holds another context")
            elif p is not None:
                if p.T >= lens[i] or tuple(ctxs[i][: p.T]) != p.key:
                    raise RuntimeError("prefill_contexts: the slot holds another prefix")
                past[i] = p.T
        if kv.ensure(slots, lens).size:  # (a scheduler has mapped them already, with room for its next steps)
            kv.release(slots[todo])  # the holds taken above: no entry stays behind unprefilled
            raise KVCapacityError("no device memory for the contexts' KV pages")
        kv.set_lens(slots, lens)
        out = torch.empty((n, self.ld), device=self.device, dtype=self.logits_dtype)
        rows = ngroups = saved = 0
        # new entries: each prefilled once, through a table of its chain's and its own pages -- the prefix entries
        # level by level, parents first, then the equal-context entries
        stages, seen = {}, set()
        for i in held:
            e = kv.slot_entry[slots[i]] or kv.slot_prefix[slots[i]]
            line = []
            while e is not None:
                line.append(e)
                e = e.parent
            for depth, e in enumerate(reversed(line)):
                if id(e) not in seen and not (e.ready if e.is_prefix else e.logits is not None):
                    seen.add(id(e))
                    stages.setdefault(depth if e.is_prefix else 1 << 30, []).append(e)
        nprefix = 0
        for depth in sorted(stages):
            new = stages[depth]
            tabs = [e.table_pages(tail=True) for e in new]
            etab = np.zeros((len(new), max(t.size for t in tabs)), dtype=np.int64)
            for j, t in enumerate(tabs):
                etab[j, : t.size] = t
            d_etab = torch.from_numpy(etab).to(self.device)
            elens = [e.T - e.past for e in new]
            for a, b in prefill_groups(elens, self.prefill_row_budget):
                lg = self._prefill_group([list(e.key[e.past:]) for e in new[a:b]], np.arange(a, b), d_etab,
                                         past=np.asarray([e.past for e in new[a:b]], dtype=np.int64),
                                         logits=not new[a].is_prefix)
                for j, e in enumerate(new[a:b]):
                    e.ready = True
                    if not e.is_prefix:
                        e.logits = lg[j:j + 1].clone()
                ngroups += 1
            rows += int(sum(elens))
            if new[0].is_prefix:
                nprefix += len(new)
            else:
                saved += int(sum(e.past for e in new))
        # singletons and private suffixes: straight into their slots' own pages
        single = np.nonzero(~sh)[0]
        if single.size:
            for a, b in prefill_groups(lens[single] - past[single], self.prefill_row_budget):
                ix = single[a:b]
                lg = self._prefill_group([ctxs[i][past[i]:] for i in ix], slots[ix], past=past[ix])
                if single.size == n:  # nothing shared: consecutive rows of the result
                    out[a:b] = lg
                else:
                    out[torch.from_numpy(ix).to(self.device)] = lg
                ngroups += 1
            rows += int((lens[single] - past[single]).sum())
            saved += int(past[single].sum())
        # holders: the master tail's rows into the first own page, the entry's logits into the slot's row
        hold = np.nonzero(sh)[0]
        if hold.size:
            self._copy_tails(slots[hold])
            out[torch.from_numpy(hold).to(self.device)] = torch.cat([kv.slot_entry[slots[i]].logits for i in hold])
        self.last_prefill = {"rows": rows, "groups": ngroups, "shared": int(hold.size)}
        if past.any() or any(kv.slot_entry[slots[i]].parent is not None for i in hold):
            self.last_prefill.update(prefix_rows_saved=saved, prefix_entries=nprefix)
        return out

    def _copy_tails(self, slots: np.ndarray) -> None:
        """``ns_kv_copy_rows`` for the holders among ``slots`` whose shared context ends inside a page."""
        from .. import _lib
        from ..coder import _stream_handle

        kv, s = self.kv, self.shape
        src, dst, rows = kv.tail_copies(slots)
        if src.size == 0:
            return
        d_src, d_dst, d_rows = (torch.from_numpy(x).to(self.device) for x in (src, dst, rows))
        _check(_lib.lib().ns_kv_copy_rows(d_src.data_ptr(), d_dst.data_ptr(), d_rows.data_ptr(), int(src.size),
                                          s.n_layer, kv.pool.layer_offset(1), s.n_head, s.n_embd // s.n_head,
                                          self._kv_format, _stream_handle()), "ns_kv_copy_rows")

    def _prefill_group(self, ctxs: List[List[int]], slots: np.ndarray, table: torch.Tensor = None, past=None,
                       logits: bool = True) -> torch.Tensor:
        """One ragged run of ``ctxs`` storing K/V through rows ``slots`` of ``table`` (default: the call's page
        table); returns the logits after each context's last token (None with ``logits`` False).  ``past``: rows of
        each sequence that its table row's first pages hold already -- ``ctxs[i]`` are then the tokens from position
        ``past[i]`` on; a run with a nonzero ``past`` goes through ``ns_seq_attention_ragged_past``."""
        from .. import _lib
        from ..coder import _stream_handle

        s, kv = self.shape, self.kv
        C, H = s.n_embd, s.n_head
        D = C // H
        L = _lib.lib()
        st = _stream_handle()
        dev = self.device
        lens = [len(c) for c in ctxs]
        seq_start, blocks = ragged_blocks(lens)
        R, n = int(seq_start[-1]), len(ctxs)
        tok = torch.from_numpy(np.concatenate([np.asarray(c, dtype=np.int32) for c in ctxs])).to(dev)
        past = np.zeros(len(ctxs), dtype=np.int32) if past is None else np.asarray(past, dtype=np.int32)
        pos = np.concatenate([np.arange(p, p + t, dtype=np.int32) for p, t in zip(past, lens)])  # past + index
        pos = torch.from_numpy(pos).to(dev)
        d_past = torch.from_numpy(past).to(dev) if past.any() else None
        d_start = torch.from_numpy(seq_start).to(dev)
        d_blocks = torch.from_numpy(blocks).to(dev)
        d_slot = torch.from_numpy(slots.astype(np.int32)).to(dev)
        table = kv.table if table is None else table

        def embed(h, a, lw0, eps):  # row positions = the token's index in its own context (% n_positions inside)
            _check(L.ns_lm_embed_ln_rows(tok.data_ptr(), self.wte.data_ptr(), self.wpe.data_ptr(), s.vocab,
                                         s.n_positions, pos.data_ptr(), h.data_ptr(), C, lw0["ln1_w"].data_ptr(),
                                         lw0["ln1_b"].data_ptr(), a.data_ptr(), C, R, C, eps, st),
                   "ns_lm_embed_ln_rows")

        def attention(i, qkv, o):
            if d_past is not None:  # continued from the pages of a shared prefix
                _check(L.ns_seq_attention_ragged_past(qkv.data_ptr(), qkv.stride(0), o.data_ptr(), o.stride(0),
                                                      d_start.data_ptr(), d_past.data_ptr(), n, R,
                                                      d_blocks.data_ptr(), blocks.shape[0], H, D, 1.0 / math.sqrt(D),
                                                      table.data_ptr(), table.stride(0), table.shape[1],
                                                      d_slot.data_ptr(), table.shape[0], kv.pool.layer_offset(i),
                                                      self._kv_format, st),
                       "ns_seq_attention_ragged_past")
                return
            _check(L.ns_seq_attention_ragged(qkv.data_ptr(), qkv.stride(0), o.data_ptr(), o.stride(0),
                                             d_start.data_ptr(), n, R, d_blocks.data_ptr(), blocks.shape[0], H, D,
                                             1.0 / math.sqrt(D), table.data_ptr(), table.stride(0), table.shape[1],
                                             d_slot.data_ptr(), table.shape[0], kv.pool.layer_offset(i),
                                             self._kv_format, st),
                   "ns_seq_attention_ragged")

        hs = self._rows_native(R, embed, attention)
        if not logits:
            return None
        last = torch.from_numpy((seq_start[1:] - 1).astype(np.int64)).to(dev)
        return self._head_native(hs.index_select(0, last))

    def _head_native(self, hrows: torch.Tensor) -> torch.Tensor:
        """ln_f + the head GEMM of ``[R, C]`` residual rows on the native kernels: ``[R, ld]`` logits."""
        from .. import _lib
        from ..coder import _stream_handle

        L = _lib.lib()
        st = _stream_handle()
        C = self.shape.n_embd
        hrows = hrows.contiguous()
        R = hrows.shape[0]
        a = torch.empty_like(hrows)
        _check(L.ns_lm_layernorm(hrows.data_ptr(), C, self.lnf_w.data_ptr(), self.lnf_b.data_ptr(), a.data_ptr(), C,
                                 R, C, float(self.shape.eps), st), "ns_lm_layernorm")
        out = torch.empty((R, self.ld), device=self.device, dtype=self.logits_dtype)
        epi = _lib.NS_LM_EPI_STORE_F32 if out.dtype == torch.float32 else _lib.NS_LM_EPI_STORE
        _check(L.ns_lm_gemm(a.data_ptr(), C, self.head_t.data_ptr(), self.head_t.stride(0), None, out.data_ptr(),
                            out.stride(0), R, self.ld, C, epi, st), "ns_lm_gemm")
        return out

    @torch.no_grad()
    def forward_packed(self, seqs: Sequence[Sequence[int]]):
        """Causal forward of whole sequences packed back to back, positions ``0..len-1`` each and no cache (the
        guard's scoring pass without padding rows; native path only): the embedding at each row's own position, the
        layer GEMMs over the ``R = sum(len)`` packed rows and ``ns_seq_attention_ragged`` in its attention-only mode
        (NULL page table: no KV page is touched).  Returns ``(h, seq_start)``: the ``[R, C]`` residual rows before
        ln_f and the int32 ``[n + 1]`` row starts.  Every kernel is row-wise or per sequence, so a sequence's rows
        have the bits :meth:`forward_sequences` gives them in any padded batch."""
        if not self.native:
            raise RuntimeError("forward_packed needs the native HIP path (fp16 on the GPU)")
        from .. import _lib
        from ..coder import _stream_handle

        s = self.shape
        C, H = s.n_embd, s.n_head
        D = C // H
        L = _lib.lib()
        st = _stream_handle()
        dev = self.device
        seqs = [[int(t) for t in q] for q in seqs]
        for q in seqs:
            if len(q) < 1:
                raise ValueError("every sequence needs at least one token")
            if len(q) > s.n_positions:
                raise ValueError(f"sequence longer than n_positions ({s.n_positions})")
            if min(q) < 0 or max(q) >= s.vocab:  # host check: never gather out of the table
                raise ValueError(f"token ids must lie in [0, {s.vocab})")
        lens = [len(q) for q in seqs]
        seq_start, blocks = ragged_blocks(lens)
        R, n = int(seq_start[-1]), len(seqs)
        tok = torch.from_numpy(np.concatenate([np.asarray(q, dtype=np.int32) for q in seqs])).to(dev)
        pos = torch.from_numpy(np.concatenate([np.arange(t, dtype=np.int32) for t in lens])).to(dev)
        d_start = torch.from_numpy(seq_start).to(dev)
        d_blocks = torch.from_numpy(blocks).to(dev)

        def embed(h, a, lw0, eps):
            _check(L.ns_lm_embed_ln_rows(tok.data_ptr(), self.wte.data_ptr(), self.wpe.data_ptr(), s.vocab,
                                         s.n_positions, pos.data_ptr(), h.data_ptr(), C, lw0["ln1_w"].data_ptr(),
                                         lw0["ln1_b"].data_ptr(), a.data_ptr(), C, R, C, eps, st),
                   "ns_lm_embed_ln_rows")

        def attention(i, qkv, o):
            _check(L.ns_seq_attention_ragged(qkv.data_ptr(), qkv.stride(0), o.data_ptr(), o.stride(0),
                                             d_start.data_ptr(), n, R, d_blocks.data_ptr(), blocks.shape[0], H, D,
                                             1.0 / math.sqrt(D), None, 0, 0, None, 0, 0, self._kv_format, st),
                   "ns_seq_attention_ragged")

        return self._rows_native(R, embed, attention), seq_start

    @torch.no_grad()
    def score_packed(self, seqs: Sequence[Sequence[int]], fused: bool = False):
        """Per-row scores of packed sequences: ``(nll, ent, seq_start)`` -- float64 device tensors ``[R]`` over the
        rows of :meth:`forward_packed`; row ``t`` of a sequence has label ``ids[t + 1]``, its last row label -1
        (``nll`` 0).  ``fused``: ln_f, then ``ns_lm_head_score`` (the head GEMM with the scores as its epilogue: no
        ``[R, V]`` logits array; the order of the softmax sums differs from ``ns_score_rows``, so the last bits do);
        where that kernel does not take the shape (``NS_ERR_UNSUPPORTED``: a K of more than one chain), and with
        ``fused`` off, the head GEMM into ``[R, ld]`` logits followed by ``ns_score_rows``."""
        from .. import _lib
        from ..coder import _stream_handle

        L = _lib.lib()
        st = _stream_handle()
        s = self.shape
        C, V, dev = s.n_embd, s.vocab, self.device
        h, seq_start = self.forward_packed(seqs)
        R = h.shape[0]
        labels = np.full(R, -1, dtype=np.int32)
        for q, a in zip(seqs, seq_start[:-1]):
            labels[a: a + len(q) - 1] = np.asarray(q[1:], dtype=np.int32)
        lab = torch.from_numpy(labels).to(dev)
        nll = torch.empty(R, dtype=torch.float64, device=dev)
        ent = torch.empty_like(nll)
        dt = _lib.NS_DTYPE_F16 if self.logits_dtype == torch.float16 else _lib.NS_DTYPE_F32
        if fused:
            a = torch.empty_like(h)
            _check(L.ns_lm_layernorm(h.data_ptr(), C, self.lnf_w.data_ptr(), self.lnf_b.data_ptr(), a.data_ptr(), C,
                                     R, C, float(s.eps), st), "ns_lm_layernorm")
            nbytes = int(L.ns_lm_head_score_work_bytes(R, V))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = L.ns_lm_head_score(a.data_ptr(), C, self.head_t.data_ptr(), self.head_t.stride(0), R, V, C, dt,
                                    lab.data_ptr(), nll.data_ptr(), ent.data_ptr(), work.data_ptr(), nbytes, st)
            if rc == 0:
                return nll, ent, seq_start
            if rc != _lib.NS_ERR_UNSUPPORTED:
                raise RuntimeError(f"ns_lm_head_score failed ({rc})")
        rows = self._head_native(h)
        _check(L.ns_score_rows(rows.data_ptr(), rows.stride(0), R, V, dt, lab.data_ptr(), nll.data_ptr(),
                               ent.data_ptr(), st), "ns_score_rows")
        return nll, ent, seq_start

    @torch.no_grad()
    def window_logits(self, ids: torch.Tensor) -> torch.Tensor:
        """Next-token logits ``[B, ld]`` of B token windows ``[B, W]`` each run from scratch with positions
        0..W-1 -- the src provider's ``_ModelAdapter`` forward over a context trimmed to ``max_context``
        (``src/neuralstego/lm/arithmetic.py:45-74``)."""
        B, W = ids.shape
        if W > self.shape.n_positions:
            raise ValueError(f"window longer than n_positions ({self.shape.n_positions})")
        if self.native:
            hs = self._seq_native(ids)
            return self._head_native(hs.view(B, W, -1)[:, -1])
        return self.forward_sequences(ids)[:, -1].contiguous()

    @torch.no_grad()
    def forward_sequences(self, ids: torch.Tensor) -> torch.Tensor:
        """Causal forward of B right-padded sequences ``[B, T]`` with positions ``0..T-1`` and no cache (the
        guard's scoring pass, ``metrics/lm_scorer.py:121-131``); returns ``[B, T, ld]`` logits in
        ``logits_dtype``.  Padding only follows the real tokens, so causality keeps it out of their rows.  fp16 on
        the GPU runs the native sequence kernels (a text's scores do not depend on the batch it is scored in)."""
        s = self.shape
        B, T = ids.shape
        if T > s.n_positions:
            raise ValueError(f"sequence longer than n_positions ({s.n_positions})")
        if self.native:
            return self._head_native(self._seq_native(ids)).view(B, T, self.ld)
        H, C = s.n_head, s.n_embd
        D = C // H
        pos = torch.arange(T, device=self.device)
        h = self.wte[ids.to(self.device).long()] + self.wpe[pos][None]
        for lw in self.layers:
            a = self._ln(h, lw["ln1_w"], lw["ln1_b"])
            qkv = torch.addmm(lw["qkv_b"], a.reshape(B * T, C), lw["qkv_w"]).view(B, T, 3, H, D)
            q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B * T, C)
            h = h + torch.addmm(lw["o_b"], o, lw["o_w"]).view(B, T, C)
            m = self._ln(h, lw["ln2_w"], lw["ln2_b"])
            f = F.gelu(torch.addmm(lw["fc_b"], m.reshape(B * T, C), lw["fc_w"]), approximate="tanh")
            h = h + torch.addmm(lw["pr_b"], f, lw["pr_w"]).view(B, T, C)
        out = self._ln(h, self.lnf_w, self.lnf_b).reshape(B * T, C) @ self.head
        out = out if out.dtype == self.logits_dtype else out.to(self.logits_dtype)
        return out.view(B, T, self.ld)

    # ------------------------------------------------------------------ paged KV (native path)
    def _pool_budget(self) -> int:
        """Device bytes the page pool may still take: free memory (with what PyTorch's allocator holds unused) less
        a 5 % reserve and :meth:`headroom_bytes` for what is allocated beside the cache."""
        free, total = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        return int(free - 0.05 * total) - self.headroom_bytes(max(self.B, 1))

    def page_pool(self, B: int = 0):
        """The page pool (created on first use; ``kv_segment_pages`` pages per segment, default from the first
        call's batch: 2B rounded up to a power of two within [64, 1024])."""
        from .kvpages import KVPagePool

        if self.pool is None:
            s = self.shape
            seg = self.kv_segment_pages
            if seg is None:
                seg = min(1024, max(64, 1 << max(0, 2 * int(B or self.B or 1) - 1).bit_length()))
            me = weakref.ref(self)  # no reference cycle: a dropped model frees its pool at once (no gc pass needed)

            def budget():
                lm = me()
                return lm._pool_budget() if lm is not None else 0

            self.pool = KVPagePool(s.n_layer, s.n_head, s.n_embd // s.n_head, self.kv_torch_dtype, self.device,
                                   budget_bytes=budget, seg_pages=seg)
        return self.pool

    def begin_slots(self, B: int, T0: int, max_new: int = 32) -> None:
        """A new call over ``B`` stream slots, every one at the shared context (cache length ``T0``): a fresh page
        table (every page of the pool free again), no page assigned yet.  ``T0 = 0``: no shared context (``kp`` /
        ``vp`` dropped) -- every stream's positions are its own (:meth:`prefill_contexts`)."""
        from .kvpages import PAGE_ROWS, PagedKV

        pool = self.page_pool(B)
        self.kv = None
        pool.reset()
        self.kv = PagedKV(pool, B, T0, (max(1, int(max_new)) + PAGE_ROWS - 1) // PAGE_ROWS + 1)
        self.B, self.L, self.T0 = int(B), int(T0), int(T0)
        if int(T0) == 0:  # no shared prefix: every position is a stream's own (prefill_contexts)
            self.kp = self.vp = None
            self.first_logits = None
        self._nb = None

    def warm_pool(self, pages: int = None, B: int = 1) -> int:
        """Grow the page pool to ``pages`` pages (default: as many as the device budget allows at batch ``B``) and
        write every new page once, so a timed call finds its pages mapped and warm (a first pass over freshly
        allocated device memory measured up to 12 % slower per step).  Returns the pool's size in pages."""
        pool = self.page_pool(B)
        saveB, self.B = self.B, max(self.B, int(B))
        try:
            want = pool.total + pool.growable_pages() if pages is None else int(pages)
            while pool.total < want and pool.growable_pages() >= pool.seg_pages:  # a segment at a time, in budget
                if not pool.add_segment(pool.seg_pages):
                    break
            for seg in pool.segments:
                seg.zero_()
        finally:
            self.B = saveB
        return pool.total

    def release_cache(self) -> None:
        """Drop the paged cache, its pool and the shared context's K/V (device memory back to PyTorch)."""
        self.kv = None
        if self.pool is not None:
            self.pool.release_memory()
        self.pool = None
        self.kp = self.vp = None
        self.k_cache = self.v_cache = None
        self._nb = None

    def _decode_native(self, tokens: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """One decode step of every slot on the batch-invariant HIP kernels: embed + ln_1 at each stream's own
        position (``lens[b] % n_positions``), then per layer c_attn GEMM, the paged KV-append attention
        (``ns_decode_attention_paged``: each stream over its own pages and length), c_proj GEMM with the residual add
        in its epilogue, ln_2, c_fc GEMM with gelu_new in its epilogue, c_proj GEMM + residual; ln_f (advancing every
        ``lens[b]`` by one) and the head GEMM straight into ``out`` ([B, ld] logits).  Every per-step quantity lives
        on the device, so the same launches are captured once as a hipGraph and replayed."""
        from .. import _lib
        from ..coder import _stream_handle

        kv = self.kv
        B = kv.B
        L = _lib.lib()
        st = _stream_handle()
        tok = tokens if tokens.dtype == torch.int32 else tokens.to(torch.int32)
        if not tok.is_contiguous() or tok.shape != (B,):
            tok = tok.reshape(B).contiguous()
        df = self.done_flags
        if df is not None and (df.dtype != torch.int32 or df.shape != (B,) or not _same_device(df.device, self.device)):
            raise ValueError(f"done_flags must be an int32 [{B}] view on {self.device}")
        done_ptr, done_stride = (df.data_ptr(), df.stride(0)) if df is not None else (None, 0)
        sl = self.stop_len
        if sl is not None and (sl.dtype != torch.int32 or sl.shape != (B,) or not sl.is_contiguous()
                               or not _same_device(sl.device, self.device)):
            raise ValueError(f"stop_len must be a contiguous int32 [{B}] tensor on {self.device}")
        stop_ptr = sl.data_ptr() if sl is not None else None
        if out.shape != (B, self.ld) or out.stride(1) != 1:
            raise ValueError(f"logits buffer must be [{B}, {self.ld}]")
        if B < 1:
            raise ValueError("decode step over an empty batch")
        s = self.shape
        C = s.n_embd
        H, D = s.n_head, C // s.n_head
        nb = self._native_buffers(B)
        h, a, qkv, o, f = (nb[k].data_ptr() for k in ("h", "a", "qkv", "o", "f"))
        ldq, ldf = nb["qkv"].stride(0), nb["f"].stride(0)
        T0 = kv.T0
        eps = float(s.eps)

        def gemm(x, ldx, wt, bias, y, ldy, epi, N, K):
            _check(L.ns_lm_gemm(x, ldx, wt.data_ptr(), wt.stride(0), bias.data_ptr() if bias is not None else None,
                                y, ldy, B, N, K, epi, st), "ns_lm_gemm")

        def ln_gemm(ln_w, ln_b, wt, bias, y, ldy, epi, N):  # ln(h) -> GEMM, one launch at small B (same bits)
            _check(L.ns_lm_ln_gemm(h, C, ln_w.data_ptr(), ln_b.data_ptr(), eps, wt.data_ptr(), wt.stride(0),
                                   bias.data_ptr(), y, ldy, B, N, C, epi, a, C, st), "ns_lm_ln_gemm")

        lens, table = kv.lens.data_ptr(), kv.table.data_ptr()
        lw0 = self.layers[0]
        _check(L.ns_lm_embed_ln_rows(tok.data_ptr(), self.wte.data_ptr(), self.wpe.data_ptr(), s.vocab,
                                     s.n_positions, lens, h, C, lw0["ln1_w"].data_ptr(), lw0["ln1_b"].data_ptr(), a,
                                     C, B, C, eps, st), "ns_lm_embed_ln_rows")
        for i, lw in enumerate(self.layers):
            if i > 0:
                ln_gemm(lw["ln1_w"], lw["ln1_b"], lw["qkv_wt"], lw["qkv_b"], qkv, ldq, _lib.NS_LM_EPI_STORE, 3 * C)
            else:  # ln_1 of layer 0 comes with the embedding
                gemm(a, C, lw["qkv_wt"], lw["qkv_b"], qkv, ldq, _lib.NS_LM_EPI_STORE, 3 * C, C)
            kp = self.kp[i, 0] if T0 else None  # [H, T0, D]
            vp = self.vp[i, 0] if T0 else None
            _check(L.ns_decode_attention_paged(qkv, ldq, table, kv.table.stride(0), kv.width,
                                               kv.pool.layer_offset(i), kp.data_ptr() if T0 else None,
                                               vp.data_ptr() if T0 else None, kp.stride(0) if T0 else 0, T0, B, H, D,
                                               lens, self.window, self._kv_format, done_ptr, done_stride, stop_ptr,
                                               o, C, 1.0 / math.sqrt(D), st), "ns_decode_attention_paged")
            gemm(o, C, lw["o_wt"], lw["o_b"], h, C, _lib.NS_LM_EPI_RESIDUAL, C, C)
            ln_gemm(lw["ln2_w"], lw["ln2_b"], lw["fc_wt"], lw["fc_b"], f, ldf, _lib.NS_LM_EPI_GELU, 4 * C)
            gemm(f, ldf, lw["pr_wt"], lw["pr_b"], h, C, _lib.NS_LM_EPI_RESIDUAL, C, 4 * C)
        # ln_f also advances every stream's cache length (no launch of its own)
        _check(L.ns_lm_layernorm_rows(h, C, self.lnf_w.data_ptr(), self.lnf_b.data_ptr(), a, C, B, C, eps, lens, st),
               "ns_lm_layernorm_rows")
        epi = _lib.NS_LM_EPI_STORE_F32 if out.dtype == torch.float32 else _lib.NS_LM_EPI_STORE
        gemm(a, C, self.head_t, None, out.data_ptr(), out.stride(0), epi, self.ld, C)
        return out

    # ------------------------------------------------------------------ graph-capturable decode step
    def begin_static(self, logits_out: torch.Tensor) -> None:
        """Prepare :meth:`step_static`: the logits go to the fixed buffer ``logits_out`` ([B, ld]) -- positions
        and cache lengths already live on the device -- so the same captured hipGraph replays every decode step.
        Needs the native HIP step (fp16 on the GPU)."""
        if not self.native:
            raise RuntimeError("graph-captured decode steps need the native HIP step (fp16 on the GPU)")
        if logits_out.shape != (self.kv.B, self.ld) or logits_out.dtype != self.logits_dtype:
            raise ValueError(f"static logits must be [{self.kv.B}, {self.ld}] {self.logits_dtype}")
        self._static_logits = logits_out

    def reserve(self, steps: int) -> bool:
        """Lockstep callers: map the pages every slot needs for the next ``steps`` decode steps (False: the device
        has no memory for them)."""
        return self.kv.ensure(np.arange(self.kv.B), self.kv.lens_host + int(steps)).size == 0  # lens_host == L, or
        # each stream's own length after prefill_contexts

    def advance(self, n: int = 1) -> None:
        """The host side of ``n`` executed decode steps (the device advanced ``lens`` itself)."""
        self.L += int(n)
        self.kv.advance(n)

    @torch.no_grad()
    def step_static(self, tokens: torch.Tensor) -> torch.Tensor:
        """:meth:`step` into the fixed logits buffer, without host-side page mapping or length bookkeeping: issues no
        host synchronisation and no allocation, so it can be captured once.  The caller maps pages ahead
        (:meth:`reserve`, or the slot scheduler) and calls :meth:`advance` per executed step."""
        self._decode_native(tokens, self._static_logits)
        return self._static_logits

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, live=None) -> torch.Tensor:
        """Feed one token per stream (``[B]`` int); position = cache length mod n_positions.  ``live`` (host bool
        ``[B]``, native path): only these streams get pages and attention this step -- a lockstep caller whose
        streams end at different lengths (the span splitter's decodes) stops paying, in memory and reads, for the
        finished ones; their logits rows are not meaningful afterwards.  ``live`` is carried to the attention as this
        step's ``stop_len``, so it cannot be combined with a caller's own ``stop_len`` (``ValueError``)."""
        B = self.B
        if tokens.shape != (B,):
            raise ValueError(f"expected {B} tokens")
        if self.native:
            from ..exceptions import KVCapacityError

            if live is not None and self.stop_len is not None:
                raise ValueError("step(live=...) would replace the stop_len that is set: use one of the two")
            if live is None:
                ok = self.reserve(1)
            else:
                live = np.asarray(live, dtype=bool).reshape(B)
                ok = self.kv.ensure(np.nonzero(live)[0], self.kv.lens_host[live] + 1).size == 0
            if not ok:
                raise KVCapacityError(f"KV cache full at {self.L} positions for B={B}: no device memory for a page")
            out = torch.empty((B, self.ld), device=self.device, dtype=self.logits_dtype)
            if live is None or live.all():
                self._decode_native(tokens, out)
            else:  # the attention skips a stream whose length reached its stop
                stop = np.where(live, np.iinfo(np.int32).max, 0).astype(np.int32)
                self.stop_len = torch.from_numpy(stop).to(self.device)
                try:
                    self._decode_native(tokens, out)
                finally:
                    self.stop_len = None
            self.advance(1)
            return out
        if self.L >= self.max_len:
            self.grow(max(64, self.max_len))
        pos = self.L % self.shape.n_positions
        h = (self.wte[tokens.long()] + self.wpe[pos])[:, None, :]
        for i in range(self.shape.n_layer):
            h = self._block(i, h, 1, causal=False)
        self.L += 1
        return self._logits(h[:, -1])

    # ------------------------------------------------------------------ several KNOWN tokens per forward (decoder)
    def _chunk_check(self, C: int) -> int:
        from .slots import check_chunk

        C = check_chunk(C)
        if not self.native:
            raise ValueError("chunked decode steps need the native HIP step (fp16 on the GPU)")
        if self.window > 0:
            raise ValueError("chunked decode steps do not support a sliding attention window")
        return C

    def _chunk_buffers(self, B: int, C: int):
        """Activation buffers of the chunked step (M = B * C rows) and its per-row cache lengths, fixed addresses."""
        cb = getattr(self, "_cb", None)
        if cb is None or cb["key"] != (B, C):
            n, dev, dt, M = self.shape.n_embd, self.device, self.dtype, B * C
            cb = self._cb = {"key": (B, C), "h": torch.empty((M, n), device=dev, dtype=dt),
                             "a": torch.empty((M, n), device=dev, dtype=dt),
                             "qkv": torch.empty((M, 3 * n), device=dev, dtype=dt),
                             "o": torch.zeros((M, n), device=dev, dtype=dt),
                             "f": torch.empty((M, 4 * n), device=dev, dtype=dt),
                             "ar": torch.arange(C, device=dev, dtype=torch.int32).unsqueeze(0),
                             "rowlens": torch.empty((B, C), device=dev, dtype=torch.int32),
                             "cnt": torch.empty((B,), device=dev, dtype=torch.int32)}
        return cb

    def _decode_chunk_native(self, tokens: torch.Tensor, counts: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """:meth:`_decode_native` over the next ``C`` tokens of every stream at once (M = B * C rows, stream b's token
        i at row b * C + i and position ``lens[b] + i``): the same launches, with ``ns_decode_attention_paged_chunk``
        -- every query the one-token kernel's arithmetic at its own key count -- as the attention, a plain ln_f and
        ``lens += counts`` as one device op.  Row (b, i) of ``out`` ([B, C, ld]) holds, for i < counts[b], the bits
        :meth:`step` returns for stream b after its tokens 0 .. i were fed one at a time; rows i >= counts[b] are not
        meaningful.  No host synchronisation, no allocation."""
        from .. import _lib
        from ..coder import _stream_handle

        kv = self.kv
        B = kv.B
        if tokens.dim() != 2 or tokens.shape[0] != B or tokens.dtype != torch.int32 or not tokens.is_contiguous():
            raise ValueError(f"tokens must be a contiguous int32 [{B}, C] tensor")
        C = self._chunk_check(tokens.shape[1])
        if counts.shape != (B,) or counts.dtype != torch.int32 or not counts.is_contiguous() or \
                not _same_device(counts.device, self.device):
            raise ValueError(f"counts must be a contiguous int32 [{B}] tensor on {self.device}")
        if out.shape != (B, C, self.ld) or not out.is_contiguous():
            raise ValueError(f"logits buffer must be a contiguous [{B}, {C}, {self.ld}] tensor")
        L = _lib.lib()
        st = _stream_handle()
        s = self.shape
        n = s.n_embd
        H, D = s.n_head, n // s.n_head
        M = B * C
        cb = self._chunk_buffers(B, C)
        h, a, qkv, o, f = (cb[k].data_ptr() for k in ("h", "a", "qkv", "o", "f"))
        ldq, ldf = cb["qkv"].stride(0), cb["f"].stride(0)
        T0 = kv.T0
        eps = float(s.eps)
        torch.add(kv.lens.unsqueeze(1), cb["ar"], out=cb["rowlens"])  # row (b, i): position lens[b] + i
        torch.clamp(counts, 0, C, out=cb["cnt"])

        def gemm(x, ldx, wt, bias, y, ldy, epi, N, K):
            _check(L.ns_lm_gemm(x, ldx, wt.data_ptr(), wt.stride(0), bias.data_ptr() if bias is not None else None,
                                y, ldy, M, N, K, epi, st), "ns_lm_gemm")

        def ln_gemm(ln_w, ln_b, wt, bias, y, ldy, epi, N):
            _check(L.ns_lm_ln_gemm(h, n, ln_w.data_ptr(), ln_b.data_ptr(), eps, wt.data_ptr(), wt.stride(0),
                                   bias.data_ptr(), y, ldy, M, N, n, epi, a, n, st), "ns_lm_ln_gemm")

        lens, table, cnt = kv.lens.data_ptr(), kv.table.data_ptr(), cb["cnt"].data_ptr()
        lw0 = self.layers[0]
        _check(L.ns_lm_embed_ln_rows(tokens.data_ptr(), self.wte.data_ptr(), self.wpe.data_ptr(), s.vocab,
                                     s.n_positions, cb["rowlens"].data_ptr(), h, n, lw0["ln1_w"].data_ptr(),
                                     lw0["ln1_b"].data_ptr(), a, n, M, n, eps, st), "ns_lm_embed_ln_rows")
        for i, lw in enumerate(self.layers):
            if i > 0:
                ln_gemm(lw["ln1_w"], lw["ln1_b"], lw["qkv_wt"], lw["qkv_b"], qkv, ldq, _lib.NS_LM_EPI_STORE, 3 * n)
            else:
                gemm(a, n, lw["qkv_wt"], lw["qkv_b"], qkv, ldq, _lib.NS_LM_EPI_STORE, 3 * n, n)
            kp = self.kp[i, 0] if T0 else None
            vp = self.vp[i, 0] if T0 else None
            _check(L.ns_decode_attention_paged_chunk(qkv, ldq, table, kv.table.stride(0), kv.width,
                                                     kv.pool.layer_offset(i), kp.data_ptr() if T0 else None,
                                                     vp.data_ptr() if T0 else None, kp.stride(0) if T0 else 0, T0, B,
                                                     H, D, lens, 0, self._kv_format, C, cnt, o, n,
                                                     1.0 / math.sqrt(D), st), "ns_decode_attention_paged_chunk")
            gemm(o, n, lw["o_wt"], lw["o_b"], h, n, _lib.NS_LM_EPI_RESIDUAL, n, n)
            ln_gemm(lw["ln2_w"], lw["ln2_b"], lw["fc_wt"], lw["fc_b"], f, ldf, _lib.NS_LM_EPI_GELU, 4 * n)
            gemm(f, ldf, lw["pr_wt"], lw["pr_b"], h, n, _lib.NS_LM_EPI_RESIDUAL, n, 4 * n)
        _check(L.ns_lm_layernorm(h, n, self.lnf_w.data_ptr(), self.lnf_b.data_ptr(), a, n, M, n, eps, st),
               "ns_lm_layernorm")
        epi = _lib.NS_LM_EPI_STORE_F32 if out.dtype == torch.float32 else _lib.NS_LM_EPI_STORE
        gemm(a, n, self.head_t, None, out.data_ptr(), out.stride(1), epi, self.ld, n)
        kv.lens.add_(cb["cnt"])  # after every layer has read the lengths
        return out

    def begin_chunk_static(self, logits_out: torch.Tensor) -> None:
        """Prepare :meth:`step_chunk_static`: the logits of ``C`` tokens per stream go to the fixed buffer
        ``logits_out`` ([B, C, ld]), so one captured hipGraph replays every chunked step."""
        if logits_out.dim() != 3:
            raise ValueError("static chunk logits must be [B, C, ld]")
        C = self._chunk_check(logits_out.shape[1])
        if logits_out.shape != (self.kv.B, C, self.ld) or logits_out.dtype != self.logits_dtype:
            raise ValueError(f"static chunk logits must be [{self.kv.B}, {C}, {self.ld}] {self.logits_dtype}")
        self._static_chunk_logits = logits_out
        self._chunk_buffers(self.kv.B, C)  # allocated here, outside any capture

    @torch.no_grad()
    def step_chunk_static(self, tokens: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        """Feed the next ``counts[b] <= C`` known tokens of every stream (``tokens`` int32 [B, C], ``counts`` int32
        [B], both on the device) in ONE forward into the :meth:`begin_chunk_static` buffer.  No host-side page
        mapping or length bookkeeping (the caller maps pages for ``lens + counts`` ahead and calls
        :meth:`advance_rows`), no host synchronisation, no allocation: capturable as a graph."""
        return self._decode_chunk_native(tokens, counts, self._static_chunk_logits)

    @torch.no_grad()
    def step_chunk(self, tokens: torch.Tensor, counts) -> torch.Tensor:
        """:meth:`step_chunk_static` with the pages reserved and the host lengths advanced here, into a fresh
        ``[B, C, ld]`` tensor (``counts``: host ints, one per stream, each in [0, C])."""
        from ..exceptions import KVCapacityError

        B = self.kv.B
        if tokens.dim() != 2 or tokens.shape[0] != B:
            raise ValueError(f"expected [{B}, C] tokens")
        C = self._chunk_check(tokens.shape[1])
        cnt = np.asarray(counts, dtype=np.int64).reshape(B)
        if (cnt < 0).any() or (cnt > C).any():
            raise ValueError(f"counts must lie in [0, {C}]")
        run = np.nonzero(cnt > 0)[0]
        if self.kv.ensure(run, self.kv.lens_host[run] + cnt[run]).size:
            raise KVCapacityError(f"KV cache full for B={B}: no device memory for a page")
        out = torch.empty((B, C, self.ld), device=self.device, dtype=self.logits_dtype)
        self._decode_chunk_native(tokens.to(device=self.device, dtype=torch.int32).contiguous(),
                                  torch.from_numpy(cnt.astype(np.int32)).to(self.device), out)
        self.advance_rows(cnt)
        return out

    def advance_rows(self, counts) -> None:
        """The host side of one executed chunked step: stream b moved ``counts[b]`` positions (:meth:`advance` with
        one count per stream)."""
        cnt = np.asarray(counts, dtype=np.int64).reshape(self.kv.B)
        self.L += int(cnt.max(initial=0))
        self.kv.advance_rows(cnt)

def ragged_blocks(lengths):
    """Host side of ``ns_seq_attention_ragged`` for sequences of ``lengths`` rows packed back to back:
    ``(seq_start, blocks)`` -- ``seq_start`` int32 ``[n + 1]``, the packed row offsets (cumulative sum), and
    ``blocks`` int32 ``[nblk, 2]``, every (sequence, 64-query block) once, longest first (a block's work grows with
    its index: it visits key blocks 0..its own), ties in sequence order."""
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lens.size == 0 or (lens < 1).any():
        raise ValueError("every sequence needs at least one row")
    if int(lens.sum()) > np.iinfo(np.int32).max:
        raise ValueError("too many packed rows")
    seq_start = np.zeros(lens.size + 1, dtype=np.int32)
    seq_start[1:] = np.cumsum(lens)
    nqb = (lens + 63) // 64
    seq = np.repeat(np.arange(lens.size, dtype=np.int64), nqb)
    blk = np.arange(seq.size, dtype=np.int64) - np.repeat(np.cumsum(nqb) - nqb, nqb)
    order = np.lexsort((seq, -blk))  # block index descending, then sequence
    blocks = np.stack([seq[order], blk[order]], axis=1).astype(np.int32)
    return seq_start, np.ascontiguousarray(blocks)


def prefill_groups(lengths, row_budget: int):
    """Split sequences of ``lengths`` rows, in order, into consecutive groups ``(first, end)`` of whole sequences
    with at most ``row_budget`` rows each; a sequence longer than the budget forms a group of its own."""
    budget = max(1, int(row_budget))
    groups, first, rows = [], 0, 0
    for i, t in enumerate(int(x) for x in lengths):
        if i > first and rows + t > budget:
            groups.append((first, i))
            first, rows = i, 0
        rows += t
    if len(lengths) > first:
        groups.append((first, len(lengths)))
    return groups


def _check(rc: int, what: str) -> None:
    """Return code of a native library call: non-zero is an error (a refused argument or a failed launch)."""
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def _normalise_device(dev: torch.device) -> torch.device:
    """``cuda`` without an index is the current device (a tensor's device always carries its index: comparing
    ``torch.device('cuda')`` with ``cuda:0`` is False)."""
    if dev.type == "cuda" and dev.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return dev


def _same_device(a: torch.device, b: torch.device) -> bool:
    return a.type == b.type and (a.index or 0) == (b.index or 0)


def random_gpt2(name: str = "gpt2", *, seed: int = 1234, **overrides):
    """Random-init GPT-2 of a named size (no network: the architecture only).  SURVEY.md §8(c)."""
    from transformers import GPT2Config, GPT2LMHeadModel

    sizes = {"gpt2": dict(n_layer=12, n_head=12, n_embd=768),
             "gpt2-medium": dict(n_layer=24, n_head=16, n_embd=1024),
             # HooshvareLab/gpt2-fa (config C4): GPT-2-small geometry with its 42,001-id Persian vocabulary
             # (unverified offline -- architecture only, random weights)
             "gpt2-fa": dict(n_layer=12, n_head=12, n_embd=768, vocab_size=42001, bos_token_id=42000,
                             eos_token_id=42000),
             "tiny": dict(n_layer=2, n_head=2, n_embd=64)}
    kw = dict(sizes[name])
    kw.update(overrides)
    torch.manual_seed(seed)
    cfg = GPT2Config(**kw)
    model = GPT2LMHeadModel(cfg)
    model.eval()
    return model
