"""One context per message: one batched call against one call per context.

    python tools/context_prefill_probe.py [--messages 256] [--payload-bytes 64] [--legs batch,percall] [--out FILE]

GPT-2-small (random weights, fp16 native path, fp16 logits), N messages of ``--payload-bytes`` bytes, N distinct contexts
of 16-128 tokens (seeded).  Two legs, each run ``--repeats`` times after one untimed pass of the same leg:

* ``batch``    ``encode_batch(bits, contexts=ctxs)``: every context prefilled ragged into its slot's own KV pages, all
               messages through one slot scheduler;
* ``percall``  what a caller without ``contexts=`` does: one ``encode_batch([bits_m], ctxs[m])`` call per message.  This
               leg uses nothing new, so it also runs on a checkout that has no ``contexts=`` (``--legs percall``).

Prints one JSON line per leg (wall seconds of every repeat, cover tokens, ``prefill_rows`` / ``prefill_groups`` of the
schedule report) and, for ``batch``, one line with the time of the ragged prefill alone (``prefill_contexts`` of all N
contexts into fresh pages, HIP events).  The two legs must give the same tokens; the tool checks it when it runs both.
"""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import random_gpt2  # noqa: E402

Q = {"temp": 0.9, "precision": 26, "topk": 300}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=256)
    ap.add_argument("--payload-bytes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="batch,percall")
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: trained-LM-like rows, ~4 bits per token)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    N = a.messages
    lm = HipArithmeticLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", logit_scale=a.scale)
    rng = np.random.default_rng(2024)
    ctxs = [[lm.vocab - 1] + rng.integers(0, lm.vocab - 1, size=int(n) - 1).tolist()
            for n in rng.integers(16, 129, size=N)]
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(9000 + s, a.payload_bytes)) for s in range(N)]
    base = {"tool": "context_prefill_probe", "library": _lib.version(), "device": torch.cuda.get_device_name(0),
            "messages": N, "payload_bytes": a.payload_bytes, "context_rows": int(sum(map(len, ctxs)))}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    tokens = {}
    if "batch" in legs:
        run = lambda: lm.encode_batch(bits, contexts=ctxs, quality=Q)  # noqa: E731
        run()
        walls = []
        for _ in range(a.repeats):
            tokens["batch"], w = timed(run)
            walls.append(round(w, 4))
        emit({"leg": "batch", "wall_s": walls, "cover_tokens": int(sum(map(len, tokens["batch"]))),
              **{k: lm.last_schedule[k] for k in ("slots", "evictions", "prefill_rows", "prefill_groups")}})
        # the ragged prefill alone: all N contexts into fresh pages
        g = lm.lm
        ms = []
        for _ in range(a.repeats + 1):
            g.begin_slots(N, 0, 64)
            lens = np.asarray([len(c) for c in ctxs])
            assert g.kv.ensure(np.arange(N), lens).size == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.prefill_contexts(ctxs, np.arange(N))
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        emit({"leg": "prefill_only", "prefill_ms": ms[1:], "first_pass_ms": ms[0], **g.last_prefill})
    if "percall" in legs:
        run = lambda: [lm.encode_batch([b], c, quality=Q)[0] for b, c in zip(bits, ctxs)]  # noqa: E731
        run()
        walls = []
        for _ in range(a.repeats):
            tokens["percall"], w = timed(run)
            walls.append(round(w, 4))
        emit({"leg": "percall", "wall_s": walls, "cover_tokens": int(sum(map(len, tokens["percall"])))})
    if len(tokens) == 2:
        assert tokens["batch"] == tokens["percall"], "the two legs disagree on a message's tokens"
        emit({"leg": "check", "same_tokens": True})
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
