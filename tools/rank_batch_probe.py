"""Rank coder, per-message contexts and qualities: one batched call against the per-packet loop.

    python tools/rank_batch_probe.py [--messages 256] [--bytes 64] [--legs batch,perpacket] [--repeats 2] [--cap]
                                     [--out FILE]

GPT-2-small (random weights, fp16 native path, fp16 logits), N messages of ``--bytes`` payload bytes with N distinct
contexts of 16-128 tokens and 8 qualities in turn over top_k, top_p, min_prob, prob_temp and temperature (``--cap``:
two of the eight carry ``cap_per_token_bits``, whose bisection is 60 passes over the row per step).  Two legs, run
alternately ``--repeats`` times after one untimed pass of each:

* ``batch``      ``encode_batch_states(bits, contexts=, qualities=)`` + ``decode_batch(tokens, contexts=, qualities=,
                 states=)``: ONE slot-scheduled call each, every context prefilled ragged into KV pages;
* ``perpacket``  what the front end did before the provider took these keywords: one
                 ``encode_batch_states([bits], context, quality=)`` and one ``decode_batch([tokens], context, quality=,
                 states=)`` per message.  This leg uses nothing new, so it also runs on a checkout without the
                 keywords (``--legs perpacket``).

Prints one JSON line per leg (wall seconds of every repeat, encode and decode apart, the SHA-256 over all tokens, and
for ``batch`` the schedule reports).  Every leg must give the same tokens and decode to the payloads; the tool checks.
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
from neuralsteganography_amd.lm.gpt2 import random_gpt2  # noqa: E402
from neuralsteganography_amd.lm.rank import HipRankLM  # noqa: E402

QUALITIES = ({"top_k": 300}, {"top_p": 0.9}, {"min_prob": 1e-5}, {"prob_temp": 0.8, "top_k": 1000}, {"temp": 0.8},
             {"top_k": 4096, "temp": 1.2}, {"top_p": 0.95, "temp": 0.9}, {"prob_temp": 1.2})
CAP_QUALITIES = ({"cap_per_token_bits": 8}, {"cap_per_token_bits": 10, "top_k": 5000})


def digest(tokens) -> str:
    h = hashlib.sha256()
    for t in tokens:
        h.update(np.asarray(t, dtype=np.int32).tobytes())
        h.update(b"|")
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="batch,perpacket")
    ap.add_argument("--cap", action="store_true", help="two of the eight qualities carry cap_per_token_bits")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    N = a.messages
    lm = HipRankLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", compute_dtype=torch.float16)
    rng = np.random.default_rng(2026)
    ctxs = [[lm.vocab - 1] + rng.integers(0, lm.vocab - 1, size=int(n) - 1).tolist()
            for n in rng.integers(16, 129, size=N)]
    payloads = [rng.integers(0, 256, size=a.bytes, dtype=np.uint8).tobytes() for _ in range(N)]
    bits = [[(b >> k) & 1 for b in p for k in range(8)] for p in payloads]
    table = list(QUALITIES)
    if a.cap:
        table[0], table[4] = CAP_QUALITIES
    quals = [dict(table[i % len(table)]) for i in range(N)]
    base = {"tool": "rank_batch_probe", "library": _lib.version(), "device": torch.cuda.get_device_name(0),
            "messages": N, "payload_bytes": a.bytes, "cap": bool(a.cap), "context_rows": int(sum(map(len, ctxs)))}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def timed(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    sched = {}

    def batch_enc():
        out = lm.encode_batch_states(bits, contexts=ctxs, qualities=quals)
        sched["encode"] = dict(lm.last_schedule)
        return out

    def batch_dec(toks, states):
        out = lm.decode_batch(toks, contexts=ctxs, qualities=quals, states=states)
        sched["decode"] = dict(lm.last_decode_schedule)
        return out

    def packet_enc():
        res = [lm.encode_batch_states([bits[i]], ctxs[i], quality=quals[i]) for i in range(N)]
        return [r[0][0] for r in res], [r[1][0] for r in res]

    def packet_dec(toks, states):
        return [lm.decode_batch([toks[i]], ctxs[i], quality=quals[i], states=[states[i]])[0] for i in range(N)]

    runs = {"batch": (batch_enc, batch_dec), "perpacket": (packet_enc, packet_dec)}
    walls = {k: {"encode_s": [], "decode_s": []} for k in legs}
    tokens = {}
    for k in legs:  # one untimed pass of each leg
        toks, states = runs[k][0]()
        assert runs[k][1](toks, states) == bits, f"{k}: the decode does not return the payloads"
    for _ in range(a.repeats):  # then the legs alternating
        for k in legs:
            (toks, states), we = timed(runs[k][0])
            out, wd = timed(runs[k][1], toks, states)
            assert out == bits, f"{k}: the decode does not return the payloads"
            tokens[k] = toks
            walls[k]["encode_s"].append(round(we, 4))
            walls[k]["decode_s"].append(round(wd, 4))
    for k in legs:
        rec = {"leg": k, **walls[k], "wall_s": [round(e + d, 4) for e, d in zip(walls[k]["encode_s"],
                                                                                 walls[k]["decode_s"])],
               "cover_tokens": int(sum(map(len, tokens[k]))), "sha256": digest(tokens[k])}
        if k == "batch":
            rec.update(schedule=sched)
        emit(rec)
    if len(tokens) == 2:
        assert digest(tokens["batch"]) == digest(tokens["perpacket"]), "the two legs disagree on a message's tokens"
        emit({"leg": "check", "same_tokens": True})
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
