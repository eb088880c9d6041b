"""A plain float64 GPT-2 and a page reader: the independent reference of ``tests/test_gpu_lm_truth.py``.

Nothing here calls the library.  ``reference_forward`` is GPT-2 written out in plain torch (float64) over the state
dict of the Hugging Face model a ``BatchedGPT2`` is built from; every weight is rounded to fp16 first and then
widened, so weight rounding is not counted as kernel error.  ``gather_kv`` reads a slot's K/V rows back out of the
native cache (the shared prefix ``kp`` / ``vp`` and the slot's pages) without mapping or writing anything.

The models, seeds and token streams of the GPU test live here too (``MODELS``, ``CASES``, ``case_streams``), so the
CPU test that proves the GPU test can discriminate (``tests/test_lm_reference_host.py``) checks the very same
constants, and so do the tolerances (``e16_of``, ``logit_tol``, ``row_tol``).
"""

from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

Ref = namedtuple("Ref", "logits K V K_exact V_exact")

FP8_MAX = 448.0


def fp8_round(x: torch.Tensor) -> torch.Tensor:
    """float64 -> fp16 -> e4m3fn (saturated to +-448 as the library's conversion saturates) -> float64."""
    h = x.to(torch.float16).clamp(-FP8_MAX, FP8_MAX)
    return h.to(torch.float8_e4m3fn).to(torch.float64)


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


@torch.no_grad()
def reference_forward(state_dict, ids, n_head, *, eps=1e-5, window=0, kv="fp16", exact_below=0, positions=None):
    """GPT-2 over one token sequence ``ids[0..T)`` in float64: ``Ref(logits[T, V], K, V, K_exact, V_exact)`` with, per
    layer, ``K[H, T, D]`` / ``V[H, T, D]`` as they enter attention.  ``logits[t]`` is what a decoder must produce
    after consuming token ``t``.  Position of row ``t`` is ``t % n_positions`` (``positions``: another list, for a
    deliberately wrong reference).

    ``window=W``: query ``t`` attends keys ``[max(0, t + 1 - W), t]`` (``include/nsg_attn.h``).

    ``kv="fp8"``: K and V are rounded to fp16, then to ``float8_e4m3fn``, and widened before attention; ``K`` / ``V``
    are those quantised values and ``K_exact`` / ``V_exact`` the float64 ones they were rounded from (equal to ``K`` /
    ``V`` for ``kv="fp16"``).  The query's OWN position is quantised too: the native decode step converts the new
    token's k and v before it stores and before it uses them (``FmtF8::from_qkv`` fills ``knew`` / ``vnew``, which
    the chunk math takes from registers at ``row == L0``, ``csrc/nsg_attn.hip``).  The native PREFILL is different:
    ``ns_seq_attention`` / ``ns_seq_attention_ragged`` attend over the fp16 c_attn output and only the stored copy is
    converted, so queries ``t < exact_below`` (the context's length) attend the exact K/V here, and no window applies
    to them either (``lm.window`` reaches the decode attention only)."""
    sd = {k: v.detach().to(torch.float16).to(torch.float64) for k, v in state_dict.items() if v.is_floating_point()}
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
    T = ids.numel()
    wte, wpe = sd["transformer.wte.weight"], sd["transformer.wpe.weight"]
    n_pos, C = wpe.shape
    H, D = n_head, C // n_head
    pos = torch.arange(T) % n_pos if positions is None else torch.as_tensor(np.asarray(positions, dtype=np.int64))
    h = wte[ids] + wpe[pos]
    t = torch.arange(T)
    causal = t[None, :] <= t[:, None]
    band = causal & (t[None, :] > t[:, None] - window) if window > 0 else causal
    prefill_row = (t < exact_below)[:, None]
    Ks, Vs, Kx, Vx = [], [], [], []
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.h."))

    def attend(q, k, v, mask):
        s = (q @ k.transpose(1, 2)) / math.sqrt(D)
        return torch.softmax(s.masked_fill(~mask, -math.inf), dim=-1) @ v

    for i in range(n_layer):
        p = f"transformer.h.{i}."
        a = _ln(h, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], eps)
        qkv = a @ sd[p + "attn.c_attn.weight"] + sd[p + "attn.c_attn.bias"]
        q, k, v = (x.view(T, H, D).transpose(0, 1) for x in qkv.split(C, dim=1))
        Kx.append(k)
        Vx.append(v)
        if kv == "fp8":
            kq, vq = fp8_round(k), fp8_round(v)
            o = torch.where(prefill_row, attend(q, k, v, causal), attend(q, kq, vq, band))
            k, v = kq, vq
        else:
            o = torch.where(prefill_row, attend(q, k, v, causal), attend(q, k, v, band)) if window > 0 else \
                attend(q, k, v, causal)
        Ks.append(k)
        Vs.append(v)
        o = o.transpose(0, 1).reshape(T, C)
        h = h + o @ sd[p + "attn.c_proj.weight"] + sd[p + "attn.c_proj.bias"]
        m = _ln(h, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], eps)
        f = _gelu_new(m @ sd[p + "mlp.c_fc.weight"] + sd[p + "mlp.c_fc.bias"])
        h = h + f @ sd[p + "mlp.c_proj.weight"] + sd[p + "mlp.c_proj.bias"]
    logits = _ln(h, sd["transformer.ln_f.weight"], sd["transformer.ln_f.bias"], eps) @ wte.t()
    return Ref(logits, Ks, Vs, Kx, Vx)


def off_by_one_positions(T, n_positions):
    """The wrong positions of the discrimination checks: right below the wrap, one too far from row ``n_positions``
    on."""
    t = np.arange(T)
    return np.where(t < n_positions, t, (t + 1) % n_positions)


# ------------------------------------------------------------------------------------------------- page reader
def gather_kv(lm, slot, layer):
    """The K and V rows ``[H, L, D]`` (float64) the native cache holds for ``slot`` at ``layer``, ``L`` the slot's
    ``kv.lens_host``.  Positions below ``kv.T0`` come from ``lm.kp`` / ``lm.vp``; the rest from the slot's row of the
    device page table, each page address resolved to (segment, page index) through ``pool.segments``,
    ``pool.block_bytes`` and ``pool.seg_pages`` (a segment is ``[n_layer, seg_pages, 2*H*32*D]``, a block
    ``[K|V][H][32][D]``).  fp8 pages (``uint8``) come back dequantised.  Reads only."""
    kv, pool = lm.kv, lm.kv.pool
    L, T0 = int(kv.lens_host[slot]), int(kv.T0)

    def widen(x):
        x = x.detach().cpu()
        return (x.view(torch.float8_e4m3fn) if x.dtype == torch.uint8 else x).to(torch.float64)

    parts_k, parts_v = [], []
    if T0:
        parts_k.append(widen(lm.kp[layer, 0][:, : min(T0, L)]))
        parts_v.append(widen(lm.vp[layer, 0][:, : min(T0, L)]))
    rows = max(0, L - T0)
    if rows:
        npg = (rows + 31) // 32
        addrs = kv.table[slot, :npg].cpu().numpy().astype(np.int64)
        where = np.full((npg, 2), -1, dtype=np.int64)
        span = pool.seg_pages * pool.block_bytes
        for si, seg in enumerate(pool.segments):
            off = addrs - seg.data_ptr()
            hit = (off >= 0) & (off < span) & (off % pool.block_bytes == 0)
            where[hit, 0], where[hit, 1] = si, off[hit] // pool.block_bytes
        if (where < 0).any():
            raise AssertionError(f"slot {slot}: page table entries {addrs[where[:, 0] < 0]} are no page of the pool")
        H = pool.block_elems // (2 * 32 * 64)
        blocks = torch.empty((npg, 2, H, 32, 64), dtype=torch.float64)
        for si in np.unique(where[:, 0]):
            sel = np.nonzero(where[:, 0] == si)[0]
            ix = torch.from_numpy(where[sel, 1]).to(pool.segments[si].device)
            blocks[torch.from_numpy(sel)] = widen(pool.segments[si][layer].index_select(0, ix)).view(-1, 2, H, 32, 64)
        for j, out in ((0, parts_k), (1, parts_v)):  # [npg, H, 32, D] -> [H, npg * 32, D]
            out.append(blocks[:, j].permute(1, 0, 2, 3).reshape(H, npg * 32, 64)[:, :rows])
    return torch.cat(parts_k, dim=1), torch.cat(parts_v, dim=1)


# ------------------------------------------------------------------------------------------------- shared constants
VOCAB, N_POS = 512, 64
MODELS = {
    "M0": dict(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, n_positions=N_POS, seed=7),
    "M1": dict(n_layer=2, n_head=12, n_embd=768, vocab_size=VOCAB, n_positions=N_POS, seed=7),
    "M2": dict(n_layer=3, n_head=2, n_embd=128, vocab_size=VOCAB, n_positions=N_POS, seed=7),
}
D_CONTEXT_LENS = [1, 31, 32, 33, 64, 65, 100, 200, 100, 33]  # the last two are copies of the 100- and 33-token ones
D_SLOT_ORDER = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]  # context i goes to slot D_SLOT_ORDER[i]
# m: the margin of section "Tolerances" of the module docstring of tests/test_gpu_lm_truth.py -- the next power of two
# above the largest measured native error / e16 (1.02, case E's window run; every case measured between 0.32 and 1.02,
# DESIGN.md section 4f), never above M_MAX.  The conditions of tests/test_lm_reference_host.py are asserted with M_MAX.
M_MAX = 8
CASES = {
    "A": dict(model="M0", ctx=37, B=3, steps=300, logits="f32", seed=101, m=2),
    "B": dict(model="M0", ctx=70, B=20, steps=40, logits="f16", seed=102, m=2),
    "C": dict(model="M0", ctx=5, B=2, steps=1040, logits="f32", seed=103, m=2),
    "D": dict(model="M0", ctx=D_CONTEXT_LENS, B=10, steps=70, logits="f32", seed=104, m=2),
    "E": dict(model="M0", ctx=37, B=3, steps=120, logits="f32", seed=105, m=2),
    "F1_3": dict(model="M1", ctx=37, B=3, steps=100, logits="f32", seed=106, m=2),
    "F1_20": dict(model="M1", ctx=37, B=20, steps=100, logits="f32", seed=107, m=2),
    "F2": dict(model="M2", ctx=37, B=3, steps=100, logits="f32", seed=108, m=2),
}
E_WINDOW = 48  # >= case E's context: the prefill (never windowed) and the windowed reference agree on its rows

_models = {}
_halves = {}


def model_of(name):
    """The Hugging Face model ``name`` of ``MODELS`` (built once per process; treat as read-only)."""
    if name not in _models:
        from neuralsteganography_amd.lm.gpt2 import random_gpt2

        kw = dict(MODELS[name])
        _models[name] = random_gpt2("tiny", seed=kw.pop("seed"), **kw)
    return _models[name]


def case_streams(name):
    """``(contexts, steps)`` of case ``name``: ``contexts[s]`` the context of stream ``s`` (one shared list repeated
    for the shared-context cases), ``steps`` int64 ``[n_steps, B]`` the teacher-forced token of every stream at every
    step.  Ids are below ``VOCAB - 1`` and differ between the streams at every step."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    B = c["B"]
    if isinstance(c["ctx"], int):
        ctx = rng.integers(0, VOCAB - 1, size=c["ctx"]).tolist()
        contexts = [ctx] * B
    else:
        contexts = [rng.integers(0, VOCAB - 1, size=n).tolist() for n in c["ctx"][:-2]]
        contexts += [list(contexts[6]), list(contexts[3])]
    base = rng.integers(0, VOCAB - 1, size=c["steps"])
    steps = (base[:, None] + 17 * np.arange(B)[None, :]) % (VOCAB - 1)  # 17 * 19 < 511: distinct per stream
    return contexts, steps.astype(np.int64)


def case_sequences(name):
    """Every stream's whole token sequence (context, then its step tokens)."""
    contexts, steps = case_streams(name)
    return [list(ctx) + steps[:, s].tolist() for s, ctx in enumerate(contexts)]


# ------------------------------------------------------------------------------------------------- tolerances
@torch.no_grad()
def hf_fp16_forward(model, ids, device="cpu"):
    """Hugging Face's own fp16 forward of one sequence on ``device`` (wrapped ``position_ids``, whole sequence):
    ``(logits[T, V], K, V)`` widened to float64 on the CPU."""
    import copy

    half = _halves.get((id(model), str(device)))
    if half is None:
        half = _halves[id(model), str(device)] = copy.deepcopy(model).half().eval().to(device)
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))[None].to(device)
    pos = (torch.arange(ids.shape[1]) % model.config.n_positions)[None].to(device)
    out = half(input_ids=ids, position_ids=pos, use_cache=True)
    K, V = past_kv(out.past_key_values)
    return out.logits[0].double().cpu(), K, V


def past_kv(past):
    """Per-layer ``K[H, T, D]`` / ``V[H, T, D]`` (float64) of a Hugging Face cache, whatever its container."""
    K, V = [], []
    layers = getattr(past, "layers", None)
    for i in range(len(layers) if layers is not None else len(past)):
        k, v = (layers[i].keys, layers[i].values) if layers is not None else past[i][:2]
        K.append(k[0].double().cpu())
        V.append(v[0].double().cpu())
    return K, V


def e16_of(model, seqs, refs, device="cpu"):
    """``(e16_logits, e16_rows)``: the largest absolute difference of Hugging Face's fp16 forward (run on ``device``)
    from the fp64 reference over ``seqs`` -- the error of an independent fp16 implementation of the same arithmetic."""
    el = er = 0.0
    done = {}
    for ids, ref in zip(seqs, refs):
        key = tuple(ids)
        if key not in done:
            lg, K, V = hf_fp16_forward(model, ids, device)
            e_l = float((lg - ref.logits).abs().max())
            e_r = max(float((a - b).abs().max()) for a, b in zip(K + V, ref.K_exact + ref.V_exact))
            done[key] = (e_l, e_r)
        el, er = max(el, done[key][0]), max(er, done[key][1])
    return el, er


def logit_tol(m, e16_logits, logits_dtype, ref_absmax):
    """``m * e16``; f16 logits add half an fp16 ulp at the largest reference logit magnitude."""
    tol = m * e16_logits
    if logits_dtype == "f16":
        tol += 0.5 * 2.0 ** (math.floor(math.log2(max(ref_absmax, 2.0 ** -14))) - 10)
    return tol


def row_tol(m, e16_rows, ref_exact=None):
    """fp16 pages: ``m * e16``.  fp8 pages (``ref_exact``: the float64 reference rows the comparison is made with):
    plus half an e4m3fn step, elementwise -- 2^-4 relative for normals, 2^-10 absolute below the normal range (2^-6)
    -- of the largest fp16 value the native row may have held, ``|ref| + m * e16``."""
    tol = m * e16_rows
    if ref_exact is None:
        return tol
    mag = ref_exact.abs() + tol
    return tol + torch.where(mag >= 2.0 ** -6, mag * 2.0 ** -4, torch.full_like(mag, 2.0 ** -10))
