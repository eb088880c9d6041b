"""Per-message sampling: one ``sample_batch`` call against one call per distinct (context, length, temperature, top-k).

    python tools/sample_batch_probe.py [--messages 256] [--legs batch,percall] [--repeats 2] [--out FILE]

GPT-2-small (random weights, fp16 native path, fp16 logits, head scale 6), N samples with N distinct contexts of 16-128
tokens, lengths spread over 32-256, 8 temperatures and top-k values {40, 300, every id} (all seeded).  Two legs, run
alternately ``--repeats`` times after one untimed pass of each:

* ``batch``    ``sample_batch(N, 0, contexts=, lengths=, temperatures=, topks=, seeds=)``: ONE slot-scheduled call
               (at most two top-k groups), every context prefilled ragged into KV pages;
* ``percall``  what a caller without these keywords does: one ``sample_batch(1, length, context, temperature=, topk=,
               seed=)`` call per distinct (context, length, temperature, top-k) -- here one per sample, since the
               contexts are distinct.  This leg uses nothing new, so it also runs on a checkout that has no
               ``contexts=`` (``--legs percall``).

Prints one JSON line per leg (wall seconds of every repeat, the SHA-256 over all tokens, and for ``batch`` the schedule
report: ``prefill_rows``, ``kv_pages_peak``, ...).  The legs must give the same tokens; the tool checks the digests when
it runs both.
"""

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import random_gpt2  # noqa: E402

TEMPS = (0.7, 0.8, 0.9, 0.95, 1.0, 1.1, 1.2, 1.3)
TOPKS = (40, 300, -1)


def digest(tokens) -> str:
    h = hashlib.sha256()
    for t in tokens:
        h.update(np.asarray(t, dtype=np.int32).tobytes())
        h.update(b"|")
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="batch,percall")
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: trained-LM-like rows)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    N = a.messages
    lm = HipArithmeticLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", logit_scale=a.scale)
    rng = np.random.default_rng(2025)
    ctxs = [[lm.vocab - 1] + rng.integers(0, lm.vocab - 1, size=int(n) - 1).tolist()
            for n in rng.integers(16, 129, size=N)]
    lens = rng.integers(32, 257, size=N).tolist()
    temps = [TEMPS[i % len(TEMPS)] for i in range(N)]
    topks = [TOPKS[(i // len(TEMPS)) % len(TOPKS)] for i in range(N)]
    seeds = [1000 + i for i in range(N)]
    base = {"tool": "sample_batch_probe", "library": _lib.version(), "device": torch.cuda.get_device_name(0),
            "messages": N, "context_rows": int(sum(map(len, ctxs))), "tokens": int(sum(lens))}
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

    def batch():
        return lm.sample_batch(N, 0, contexts=ctxs, lengths=lens, temperatures=temps, topks=topks, seeds=seeds)[0]

    def percall():
        return [lm.sample_batch(1, lens[i], ctxs[i], temperature=temps[i], topk=topks[i], seed=seeds[i])[0][0]
                for i in range(N)]

    runs = {"batch": batch, "percall": percall}
    walls = {k: [] for k in legs}
    tokens = {}
    for k in legs:  # one untimed pass of each leg
        runs[k]()
    for _ in range(a.repeats):  # then the legs alternating
        for k in legs:
            tokens[k], w = timed(runs[k])
            walls[k].append(round(w, 4))
            if k == "batch":
                sched = dict(lm.last_sample_schedule)
    for k in legs:
        rec = {"leg": k, "wall_s": walls[k], "sha256": digest(tokens[k])}
        if k == "batch":
            rec.update(sched)
        emit(rec)
    if len(tokens) == 2:
        assert digest(tokens["batch"]) == digest(tokens["percall"]), "the two legs disagree on a sample's tokens"
        emit({"leg": "check", "same_tokens": True})
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
