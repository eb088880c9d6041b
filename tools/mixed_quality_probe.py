"""Per-message coder quality: one ``encode_batch(qualities=...)`` call against one call per distinct quality.

GPT-2-small (random-init weights, fp16 compute and logits, head scaled x6: trained-entropy rows), 256 messages of 64
bytes from one 32-token context, 8 distinct qualities (top-k 60 to 300, temperature 0.7 to 1.0, precision 16 and 26),
message m carrying quality m mod 8.  Leg ``mixed``: all 256 messages in one call, every stream reading its row of the
quality table.  Leg ``grouped``: what a caller did before library 0.31 -- one call per distinct quality over that
quality's 32 messages, each with its own small batch, prefill and slot pool.  One untimed run of each leg, then
``--runs`` timed ones with the legs alternating; both legs must give the same tokens.  ``--legs grouped`` alone runs
on a tree without ``qualities=`` (the parent commit's time for the second leg).  Prints one JSON line per timed run
and a summary line; ``--out`` appends them to a file.  Payload seeds start at ``--seed0`` = 1000: with seeds from 0,
message 152 (top-k 60, temperature 0.7, precision 16) stalls the coder -- alone on the one-quality path as well: the
reference's coder has no underflow handling, and at precision 16 a narrow interval astride the midpoint is not rare.

``--wide``: 8 qualities of top-k 50,000 (the api default, beyond the single-pass limit: the wide kernels), temperature
0.7 to 1.3, precision 16, 20 and 26.  Leg ``mixed`` is then one call whose wide step reads every stream's row
(``ns_set_stream_quality_wide``); leg ``switch_off`` the same call with ``mix_wide_qualities = False`` (one call per
distinct quality inside ``encode_batch``: what the call did before); leg ``grouped`` as above.  Every leg's tokens must
have the same SHA-256, printed in the summary.
usage: python tools/mixed_quality_probe.py [--wide] [--messages 256] [--bytes 64] [--runs 2]
                                           [--legs mixed,grouped[,switch_off]] [--out F]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

QUALITIES = [{"topk": 60, "temp": 0.7, "precision": 16}, {"topk": 100, "temp": 0.8, "precision": 26},
             {"topk": 140, "temp": 0.9, "precision": 16}, {"topk": 180, "temp": 1.0, "precision": 26},
             {"topk": 220, "temp": 0.7, "precision": 26}, {"topk": 260, "temp": 0.8, "precision": 16},
             {"topk": 300, "temp": 0.9, "precision": 26}, {"topk": 300, "temp": 1.0, "precision": 16}]
WIDE_QUALITIES = [{"topk": 50000, "temp": 0.7, "precision": 16}, {"topk": 50000, "temp": 0.8, "precision": 20},
                  {"topk": 50000, "temp": 0.9, "precision": 26}, {"topk": 50000, "temp": 1.0, "precision": 16},
                  {"topk": 50000, "temp": 1.1, "precision": 20}, {"topk": 50000, "temp": 1.2, "precision": 26},
                  {"topk": 50000, "temp": 1.3, "precision": 16}, {"topk": 50000, "temp": 1.0, "precision": 26}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=64)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: about 4.2 bits per token)")
    ap.add_argument("--seed0", type=int, default=1000, help="first payload seed (message s carries seed0 + s)")
    ap.add_argument("--wide", action="store_true", help="top-k 50,000 qualities (the wide kernels)")
    ap.add_argument("--legs", default=None, help="default: mixed,grouped; with --wide also switch_off")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import hashlib

    import torch

    from neuralsteganography_amd import _lib, synthetic
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    legs = [x for x in (args.legs or ("mixed,switch_off,grouped" if args.wide else "mixed,grouped")).split(",") if x]
    qualities = WIDE_QUALITIES if args.wide else QUALITIES
    N, nq = args.messages, len(qualities)
    lm = HipArithmeticLM(random_gpt2("gpt2"), None, device="cuda:0", logits_dtype="f16", max_batch=N,
                         logit_scale=args.scale)
    context = [lm.vocab - 1] + list(synthetic.DEFAULT_CONTEXT[1:])
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(args.seed0 + s, args.bytes)) for s in range(N)]
    qs = [qualities[m % nq] for m in range(N)]

    def mixed():
        return lm.encode_batch(bits, context, qualities=qs)

    def grouped():
        out = [None] * N
        for g in range(nq):
            members = list(range(g, N, nq))
            for m, toks in zip(members, lm.encode_batch([bits[m] for m in members], context, quality=qualities[g])):
                out[m] = toks
        return out

    def switch_off():
        lm.mix_wide_qualities = False
        try:
            return mixed()
        finally:
            lm.mix_wide_qualities = True

    fns = {"mixed": mixed, "grouped": grouped, "switch_off": switch_off}

    def sha(toks):
        return hashlib.sha256(json.dumps(toks).encode()).hexdigest()

    def timed(name):
        lm.drain_states()
        lm._decode_states.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = fns[name]()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    lines = []
    ref = {name: timed(name)[1] for name in legs}  # untimed: warms kernels, pools and coder contexts up
    assert len({sha(t) for t in ref.values()}) == 1, "the legs gave different tokens"
    secs = {name: [] for name in legs}
    for r in range(args.runs):
        for name in legs:
            s, toks = timed(name)
            assert toks == ref[name], f"{name}: run {r} gave other tokens than the untimed run"
            secs[name].append(s)
            lines.append({"leg": name, "run": r, "seconds": s})
    ntok = sum(len(t) for t in ref[legs[0]])
    summary = {"library": _lib.version(), "messages": N, "payload_bytes": args.bytes, "distinct_qualities": nq,
               "cover_tokens": ntok, "head_scale": args.scale, "wide": bool(args.wide),
               "token_sha256": sha(ref[legs[0]]),
               "seconds_mean": {k: sum(v) / len(v) for k, v in secs.items()}, "same_tokens": len(legs) >= 2 or None}
    if "switch_off" in secs and "mixed" in secs:
        summary["switch_off_over_mixed"] = summary["seconds_mean"]["switch_off"] / summary["seconds_mean"]["mixed"]
    if "grouped" in secs and "mixed" in secs:
        summary["grouped_over_mixed"] = summary["seconds_mean"]["grouped"] / summary["seconds_mean"]["mixed"]
    lines.append(summary)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
