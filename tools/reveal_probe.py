"""Reveal many cover texts with per-text seeds and qualities: one slot-scheduled call against one call per
distinct (seed, quality).

GPT-2-small (random-init weights, fp16 compute and logits, head scaled x6: trained-entropy rows) behind the id-exact
``IdTokenizer``; ``--covers`` secrets of ``--secret-bytes`` bytes, ``--chunk-bytes`` small enough for at least three
spans a cover, ``ecc="none"``; ``--seeds`` distinct seeds of 16-128 tokens; six qualities, those ``iter_attempts``
pairs: the base (top-k 300, temp 0.9, precision 26), the default schedule's (80, 0.8), (70, 0.7) and (60, base temp),
and the schedule with its temperature steps reversed, (80, 0.7) and (70, 0.8).  Cover i carries seed ``i % seeds`` and
quality ``i % 6``; the covers are generated once, per quality, untimed.

Legs (``--legs``, run alternately: one untimed run of each, then ``--runs`` timed ones of each):
  slots     one ``cover_reveal_batch(attempts=...)`` call (the slot-scheduled batch, ``--slots`` slots);
  existing  one ``cover_reveal_batch(seed_text=, quality=)`` call per distinct (seed, quality) -- it uses nothing this
            build added, so the same file run from a checkout of the parent commit with ``--legs existing`` is the
            parent's time.
Every run's secrets are asserted equal to the secrets hidden; the untimed run also collects every text's spans, and
the SHA-256 over all spans and secrets is printed per leg (it must be equal across legs and trees).  Prints one JSON
line per run as it ends and a summary line per leg; ``--out`` appends them to a file.
usage: python tools/reveal_probe.py [--covers 256] [--seeds 16] [--secret-bytes 64] [--chunk-bytes 24]
                                    [--legs slots,existing] [--slots N] [--runs 2] [--out F]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BASE = {"temp": 0.9, "precision": 26, "topk": 300, "finish_sent": False}


def qualities():
    """The six override sets, from ``iter_attempts`` itself."""
    from neuralsteganography_amd.cover import DEFAULT_REGEN_STRATEGY, iter_attempts

    rev = dict(DEFAULT_REGEN_STRATEGY, temperature_steps=list(reversed(DEFAULT_REGEN_STRATEGY["temperature_steps"])))
    out = []
    for strategy in (DEFAULT_REGEN_STRATEGY, rev):
        for a in iter_attempts("", 3, strategy):
            if a.overrides not in out:
                out.append(dict(a.overrides))
    assert len(out) == 6, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--covers", type=int, default=256)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--secret-bytes", type=int, default=64)
    ap.add_argument("--chunk-bytes", type=int, default=24)
    ap.add_argument("--legs", default="slots,existing")
    ap.add_argument("--slots", type=int, default=None)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: about 4.2 bits per token)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from neuralsteganography_amd import _lib, cover, stego, synthetic
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    stego.make_msg_id = lambda: "00000000-0000-4000-8000-000000000001"  # the same covers in every tree and run
    N, legs = args.covers, [x for x in args.legs.split(",") if x]
    tok = synthetic.IdTokenizer(50257)
    lm = HipArithmeticLM(random_gpt2("gpt2"), tok, device="cuda:0", logits_dtype="f16", max_batch=N,
                         logit_scale=args.scale)
    rng = np.random.default_rng(20)
    seed_pool = [tok.decode([int(t) for t in rng.integers(4, 50000, size=int(n)) if t != 628]).strip()
                 for n in np.linspace(16, 128, args.seeds).astype(int)]
    overrides = qualities()
    seeds = [seed_pool[i % args.seeds] for i in range(N)]
    over = [overrides[i % 6] for i in range(N)]
    merged = [{**stego.normalise_quality(BASE), **stego.normalise_quality(o)} for o in over]
    secrets = [synthetic.payload_bytes(4000 + i, args.secret_bytes) for i in range(N)]
    texts = [None] * N
    for k in range(6):
        members = [i for i in range(N) if i % 6 == k]
        if members:
            got = cover.cover_generate_batch([secrets[i] for i in members], seed_texts=[seeds[i] for i in members],
                                             quality=merged[members[0]], ecc="none", chunk_bytes=args.chunk_bytes,
                                             quality_gate=False, lm=lm)
            for i, t in zip(members, got):
                texts[i] = t
    pairs = {}
    for i in range(N):
        pairs.setdefault((seeds[i], i % 6), []).append(i)

    def run_slots(with_spans):
        atts = [cover.Attempt(seeds[i], over[i], "probe") for i in range(N)]
        kw = {} if args.slots is None else {"slots": args.slots}
        spans = cover.texts_to_spans(texts, seed_texts=seeds, qualities=merged, lm=lm, **kw) if with_spans else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cover.cover_reveal_batch(texts, attempts=atts, quality=BASE, ecc="none", lm=lm, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, spans, dict(lm.last_reveal_schedule)

    def run_existing(with_spans):
        out, spans, secs = [None] * N, [None] * N, 0.0
        for (seed, k), members in pairs.items():
            sub = [texts[i] for i in members]
            if with_spans:
                for i, sp in zip(members, cover.texts_to_spans(sub, seed_text=seed, quality=merged[members[0]], lm=lm)):
                    spans[i] = sp
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = cover.cover_reveal_batch(sub, seed_text=seed, quality=merged[members[0]], ecc="none", lm=lm)
            torch.cuda.synchronize()
            secs += time.perf_counter() - t0
            for i, s in zip(members, got):
                out[i] = s
        return secs, out, (spans if with_spans else None), {"calls": len(pairs)}

    runner = {"slots": run_slots, "existing": run_existing}
    digest, sched, secs = {}, {}, {leg: [] for leg in legs}
    lines = []
    for leg in legs:  # untimed: warms kernels, pools and coder contexts up, and collects the spans
        _, out, spans, sched[leg] = runner[leg](True)
        assert out == secrets, f"{leg}: revealed secrets differ from the secrets hidden"
        assert all(len(sp) >= 3 for sp in spans), "fewer than three spans in a cover: lower --chunk-bytes"
        digest[leg] = hashlib.sha256(json.dumps([spans, [s.hex() for s in out]]).encode()).hexdigest()
        print(json.dumps({"leg": leg, "untimed": True, "sha256_spans_and_secrets": digest[leg]}), flush=True)
    for r in range(args.runs):
        for leg in legs:
            s, out, _, sched[leg] = runner[leg](False)
            assert out == secrets, f"{leg}: revealed secrets differ from the secrets hidden"
            secs[leg].append(s)
            lines.append({"leg": leg, "run": r, "seconds": s})
            print(json.dumps(lines[-1]), flush=True)
    done = len(lines)
    ntok = sum(len(tok.encode(t)) for t in texts)
    for leg in legs:
        v = secs[leg]
        lines.append({"leg": leg, "library": _lib.version(), "covers": N, "seeds": args.seeds, "pairs": len(pairs),
                      "secret_bytes": args.secret_bytes, "chunk_bytes": args.chunk_bytes, "text_tokens": ntok,
                      "head_scale": args.scale, "slots": args.slots, "seconds_mean": sum(v) / len(v),
                      "spread": (max(v) - min(v)) / (sum(v) / len(v)), "schedule": sched[leg],
                      "sha256_spans_and_secrets": digest[leg]})
    print("\n".join(json.dumps(x) for x in lines[done:]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
