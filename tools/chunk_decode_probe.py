"""Decode known covers several tokens per forward: ``decode_batch(..., chunk=C)`` against ``chunk=1``.

GPT-2-small (random-init weights, fp16 compute and logits, head scaled x6: trained-entropy rows), ``--messages``
payloads of ``--bytes`` bytes from one 32-token context, encoded once; then ``decode_batch`` over the same covers
through ``--slots`` slots (fewer than messages: slots are refilled) at every ``chunk`` of ``--chunks``.  Per setting
one untimed run, then ``--runs`` timed ones; the decoded bits are asserted equal to the payloads at every setting and
run.  ``--chunks 1`` runs on a tree without ``chunk=`` (the parent commit's time: the yardstick) -- the keyword is
only passed when it is not 1.  Prints one JSON line per timed run and a summary line; ``--out`` appends them to a
file.
usage: python tools/chunk_decode_probe.py [--messages 384] [--bytes 256] [--slots 128] [--chunks 1,2,4,8,16]
                                          [--runs 2] [--out F]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=384)
    ap.add_argument("--bytes", type=int, default=256)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--chunks", default="1,2,4,8,16")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: about 4.2 bits per token)")
    ap.add_argument("--seed0", type=int, default=1000, help="first payload seed (message s carries seed0 + s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from neuralsteganography_amd import _lib, synthetic
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    N = args.messages
    chunks = [int(x) for x in args.chunks.split(",") if x]
    quality = {"topk": 300, "temp": 0.9, "precision": 26}
    lm = HipArithmeticLM(random_gpt2("gpt2"), None, device="cuda:0", logits_dtype="f16", max_batch=N,
                         logit_scale=args.scale)
    context = [lm.vocab - 1] + list(synthetic.DEFAULT_CONTEXT[1:])
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(args.seed0 + s, args.bytes)) for s in range(N)]
    covers = lm.encode_batch(bits, context, quality=quality)
    ntok = sum(len(c) for c in covers)

    def timed(C):
        kw = {"chunk": C} if C != 1 else {}
        lm._decode_states.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = lm.decode_batch(covers, context, quality=quality, slots=args.slots, **kw)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        assert all(o[: len(b)] == b for o, b in zip(out, bits)), f"chunk={C}: decoded bits differ from the payloads"
        return s

    lines, secs = [], {}
    for C in chunks:
        timed(C)  # untimed: warms kernels, pools and coder contexts up
        secs[C] = [timed(C) for _ in range(args.runs)]
        for r, s in enumerate(secs[C]):
            lines.append({"chunk": C, "run": r, "seconds": s, "tokens_per_second": ntok / s})
    summary = {"library": _lib.version(), "messages": N, "payload_bytes": args.bytes, "slots": args.slots,
               "cover_tokens": ntok, "longest_cover": max(len(c) for c in covers), "head_scale": args.scale,
               "seconds_mean": {str(C): sum(v) / len(v) for C, v in secs.items()},
               "spread": {str(C): (max(v) - min(v)) / (sum(v) / len(v)) for C, v in secs.items()},
               "bits_equal_payloads": True}
    lines.append(summary)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
