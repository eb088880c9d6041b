"""Messages that carry the same context: shared KV pages against one private copy per message.

    python tools/context_share_probe.py [--contexts 16] [--copies 16] [--payload-bytes 64] [--legs on,off] [--out FILE]

GPT-2-small (random weights, fp16 native path, fp16 logits, head scale 6), ``--contexts`` distinct contexts of 256 to
1,022 tokens (seeded), each carried by ``--copies`` messages of ``--payload-bytes`` bytes (the shape of
``stego_encode_batch(messages, seed_texts=...)``: every packet of a message is a stream with the message's seed as
its context), interleaved so that equal contexts are not neighbours.  Legs, run alternating ``--repeats`` times after
one untimed pass of each:

* ``on``   ``encode_batch(bits, contexts=ctxs)`` with ``share_contexts`` on: every context prefilled once, its full
           pages shared by its messages (``lm/kvpages.py``);
* ``off``  the same call with ``share_contexts`` off: every message prefills and keeps its own copy.

On a checkout that has no ``share_contexts`` the tool runs the one leg it can, ``base`` (the plain call), so the same
file measures the parent commit.  Prints one JSON line per leg: the wall seconds of every repeat, ``prefill_rows``,
``kv_pages_peak``, the cover tokens and a SHA-256 of all tokens (equal digests: the legs, and the builds, give the same
tokens), and with two legs one line saying whether their tokens are equal.
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

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import random_gpt2  # noqa: E402

Q = {"temp": 0.9, "precision": 26, "topk": 300}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=16)
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--payload-bytes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="on,off")
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: trained-LM-like rows, ~4 bits per token)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    has_switch = hasattr(HipArithmeticLM, "share_contexts")
    legs = a.legs.split(",") if has_switch else ["base"]
    lm = HipArithmeticLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", logit_scale=a.scale)
    rng = np.random.default_rng(2025)
    distinct = [[lm.vocab - 1] + rng.integers(0, lm.vocab - 1, size=int(n) - 1).tolist()
                for n in rng.integers(256, 1023, size=a.contexts)]
    N = a.contexts * a.copies
    ctxs = [distinct[m % a.contexts] for m in range(N)]  # copy j of context i is message j * contexts + i
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(9000 + s, a.payload_bytes)) for s in range(N)]
    base = {"tool": "context_share_probe", "library": _lib.version(), "device": torch.cuda.get_device_name(0),
            "contexts": a.contexts, "copies": a.copies, "payload_bytes": a.payload_bytes,
            "context_rows_distinct": int(sum(map(len, distinct))), "context_rows_all": int(sum(map(len, ctxs)))}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def run(leg):
        if has_switch:
            lm.share_contexts = leg == "on"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = lm.encode_batch(bits, contexts=ctxs, quality=Q)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for leg in legs:  # one untimed pass of each: pages mapped and warm, graphs' kernels loaded
        run(leg)
    walls = {leg: [] for leg in legs}
    tokens, sched = {}, {}
    for _ in range(a.repeats):
        for leg in legs:  # alternating
            tokens[leg], w = run(leg)
            walls[leg].append(round(w, 4))
            sched[leg] = dict(lm.last_schedule)
    for leg in legs:
        digest = hashlib.sha256(json.dumps(tokens[leg]).encode()).hexdigest()
        keys = ("slots", "evictions", "prefill_rows", "prefill_groups", "prefill_shared", "kv_pages_peak")
        emit({"leg": leg, "wall_s": walls[leg], "cover_tokens": int(sum(map(len, tokens[leg]))),
              "tokens_sha256": digest, **{k: sched[leg][k] for k in keys if k in sched[leg]}})
    if len(legs) == 2:
        same = tokens[legs[0]] == tokens[legs[1]]
        emit({"leg": "check", "same_tokens": same})
        assert same, "the two legs disagree on a message's tokens"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
