"""Decode-step probe of the batch-invariant GPT-2 kernels (include/nsg_lm.h) vs the PyTorch / hipBLASLt ops.

For one batch size B: each GEMM of a decode step (c_attn, attn c_proj, c_fc, mlp c_proj, lm head) timed on
ns_lm_gemm and on torch.addmm/matmul (TFLOP/s), and a layer norm.  HIP events on the launch stream; prints JSON
lines.  The decode attention is timed by tools/paged_attn_probe.py (paged and dense layouts).
--cold: each GEMM cycles over enough distinct operand sets (activations, weights, output) to exceed the 256 MiB
Infinity Cache, so every launch finds its operands in HBM as it does inside a decode step, where a layer's weights
and activations were last touched a whole step ago; without it the launches re-read hot buffers.
usage: python tools/lm_probe.py [--batch 4096] [--model gpt2] [--reps 20] [--configs] [--cold]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", action="store_true", help="time every ns_lm_gemm_config tile configuration")
    ap.add_argument("--cold", action="store_true", help="cycle over operand sets larger than the Infinity Cache")
    args = ap.parse_args()
    import torch

    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _stream_handle
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2

    dev = torch.device("cuda", 0)
    B = args.batch
    L = _lib.lib()

    def timed(fn, reps=args.reps):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    lm = BatchedGPT2(random_gpt2(args.model), device=dev, logits_dtype=torch.float16)
    s = lm.shape
    C = s.n_embd
    lw = lm.layers[0]
    x = torch.randn((B, 4 * C), device=dev).half()
    shapes = [("c_attn", lw["qkv_wt"], lw["qkv_b"], lw["qkv_w"], C, 0), ("attn_proj", lw["o_wt"], lw["o_b"], lw["o_w"], C, 2),
              ("c_fc", lw["fc_wt"], lw["fc_b"], lw["fc_w"], C, 1), ("mlp_proj", lw["pr_wt"], lw["pr_b"], lw["pr_w"], 4 * C, 2),
              ("lm_head", lm.head_t, None, lm.head, C, 0)]
    # the same shapes with a plain store (the epilogue's own cost) and the fp32-logits head the bench's coder reads
    shapes += [("c_fc_store", lw["fc_wt"], lw["fc_b"], lw["fc_w"], C, 0), ("lm_head_f32", lm.head_t, None, lm.head, C, 3)]
    for name, wt, bias, w, K, epi in shapes:
        N = wt.shape[0]
        xa = x[:, :K].contiguous()
        y = torch.empty((B, N), device=dev, dtype=torch.float32 if epi == 3 else torch.float16)
        st = _stream_handle()
        bp = bias.data_ptr() if bias is not None else None
        # operand sets: one (hot), or as many copies as exceed the cache with one to spare (cold)
        set_bytes = xa.nbytes + wt.nbytes + y.nbytes
        nsets = 2 + (320 << 20) // set_bytes if args.cold else 1
        sets = [(xa, wt, w, y)] + [(xa.clone(), wt.clone(), w.clone(), torch.empty_like(y)) for _ in range(nsets - 1)]
        turn = [0]

        def next_set():
            turn[0] = (turn[0] + 1) % nsets
            return sets[turn[0]]

        def native():
            xs, ws, _, ys = next_set()
            rc = L.ns_lm_gemm(xs.data_ptr(), K, ws.data_ptr(), K, bp, ys.data_ptr(), N, B, N, K, epi, st)
            assert rc == 0

        def ref():
            xs, _, wr, _ = next_set()
            if bias is not None:
                return torch.addmm(bias, xs, wr)
            return xs @ wr

        ms_n, ms_t = timed(native), timed(ref)
        fl = 2.0 * B * N * K
        rec = {"gemm": name, "M": B, "N": N, "K": K, "operand_sets": nsets, "ms_native": ms_n, "ms_torch": ms_t,
               "tflops_native": fl / ms_n / 1e9, "tflops_torch": fl / ms_t / 1e9}
        if args.configs:
            per = {}
            for cfg in range(L.ns_lm_gemm_configs()):
                if cfg < 3 and B > 256:
                    continue  # direct (small-batch) kernels re-read the weights per 64 rows

                def one(cfg=cfg):
                    xs, ws, _, ys = next_set()
                    rc = L.ns_lm_gemm_config(xs.data_ptr(), K, ws.data_ptr(), K, bp, ys.data_ptr(), N, B, N, K, epi,
                                             cfg, st)
                    assert rc == 0

                per[cfg] = round(fl / timed(one) / 1e9, 1)
            rec["tflops_by_config"] = per
        print(json.dumps(rec), flush=True)
    a = torch.randn((B, C), device=dev).half()
    ln_out = torch.empty_like(a)

    def ln():
        L.ns_lm_layernorm(a.data_ptr(), C, lw["ln1_w"].data_ptr(), lw["ln1_b"].data_ptr(), ln_out.data_ptr(), C, B, C,
                          1e-5, _stream_handle())

    ms_ln = timed(ln)
    ms_ln_t = timed(lambda: torch.nn.functional.layer_norm(a, (C,), lw["ln1_w"], lw["ln1_b"], 1e-5))
    print(json.dumps({"layernorm": C, "M": B, "ms_native": ms_ln, "ms_torch": ms_ln_t,
                      "GBs_native": 2 * B * C * 2 / ms_ln / 1e6}), flush=True)


if __name__ == "__main__":
    main()
