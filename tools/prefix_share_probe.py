"""Contexts that begin alike: the common prefix's KV pages shared against one whole prefill and copy per context.

    python tools/prefix_share_probe.py [--prefixes 16] [--suffixes 16] [--prefix-tokens 512] [--payload-bytes 64]
                                       [--legs on,off] [--out FILE]

GPT-2-small (random weights, fp16 native path, fp16 logits, head scale 6), ``--prefixes`` distinct prefixes of
``--prefix-tokens`` tokens (seeded), each followed by ``--suffixes`` distinct suffixes of 16 to 128 tokens: one message
of ``--payload-bytes`` bytes per context, all contexts distinct (a conversation history with a different last line per
recipient; one preamble with a topic per message), interleaved so that contexts of one prefix are not neighbours.
Legs, run alternating ``--repeats`` times after one untimed pass of each:

* ``on``   ``encode_batch(bits, contexts=ctxs)`` with ``share_prefixes`` on: every prefix prefilled once, in 64-row
           blocks, its pages shared by the contexts that begin with it (``lm/kvpages.py``);
* ``off``  the same call with ``share_prefixes`` off: every context is prefilled whole into pages of its own.

On a checkout that has no ``share_prefixes`` the tool runs the one leg it can, ``base`` (the plain call), so the same
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
    ap.add_argument("--prefixes", type=int, default=16)
    ap.add_argument("--suffixes", type=int, default=16)
    ap.add_argument("--prefix-tokens", type=int, default=512)
    ap.add_argument("--payload-bytes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="on,off")
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: trained-LM-like rows, ~4 bits per token)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    has_switch = hasattr(HipArithmeticLM, "share_prefixes")
    legs = a.legs.split(",") if has_switch else ["base"]
    lm = HipArithmeticLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", logit_scale=a.scale)
    rng = np.random.default_rng(2026)
    heads = [[lm.vocab - 1] + rng.integers(0, lm.vocab - 1, size=a.prefix_tokens - 1).tolist()
             for _ in range(a.prefixes)]
    N = a.prefixes * a.suffixes
    # suffix j of prefix i is message j * prefixes + i; every suffix is drawn anew, so all N contexts are distinct
    ctxs = [heads[m % a.prefixes] + rng.integers(0, lm.vocab - 1, size=int(rng.integers(16, 129))).tolist()
            for m in range(N)]
    assert len({tuple(c) for c in ctxs}) == N
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(9000 + s, a.payload_bytes)) for s in range(N)]
    base = {"tool": "prefix_share_probe", "library": _lib.version(), "device": torch.cuda.get_device_name(0),
            "prefixes": a.prefixes, "suffixes": a.suffixes, "prefix_tokens": a.prefix_tokens,
            "payload_bytes": a.payload_bytes, "context_rows_all": int(sum(map(len, ctxs)))}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def run(leg):
        if has_switch:
            lm.share_prefixes = leg == "on"
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
        keys = ("slots", "evictions", "prefill_rows", "prefill_groups", "prefill_shared", "kv_pages_peak",
                "prefix_rows_saved", "prefix_entries")
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
