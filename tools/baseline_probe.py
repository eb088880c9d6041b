"""Time one encode step of the baseline coders beside the arithmetic coder's, in one process.

B = 4,096 streams, V = 50,257, fp16 rows (random normal x 3): ``ns_huffman_encode_step`` and ``ns_bins_encode_step`` at
block 3 and 8, and ``ns_encode_step`` at top-k 300 (precision 26, temperature 0.9).  The legs alternate; every leg
runs ``--steps`` steps three times, the first untimed.  Prints one JSON record per leg (microseconds per step of the
two timed runs) and, with ``--out``, writes them to that file.

    python tools/baseline_probe.py --out profiles/r21/baseline_probe.json
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> None:
    import numpy as np
    import torch

    from neuralsteganography_amd.coder import (BaselineEncodeSession, CoderContext, CoderParams, EncodeSession,
                                               row_stride)

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=50257)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, V = a.batch, a.vocab
    ld = row_stride(V, "f16")
    gen = torch.Generator(device="cuda").manual_seed(21)
    logits = (torch.randn((B, ld), generator=gen, device="cuda") * 3.0).to(torch.float16)
    rng = np.random.default_rng(21)
    nbits = 64 * a.steps * 3  # no stream runs out of payload (a block-8 Huffman code is at most 255 bits, ~8 typical)
    bits = [rng.integers(0, 2, size=nbits, dtype=np.uint8) for _ in range(B)]

    legs = {}
    base = CoderContext(CoderParams(vocab=V, dtype="f16", topk=2), max_batch=B)
    for mode in ("huffman", "bins"):
        for block in (3, 8):
            legs[f"{mode}_block{block}"] = BaselineEncodeSession(base, bits, mode=mode, block_size=block,
                                                                 max_tokens=4 * a.steps)
    arith = CoderContext(CoderParams(vocab=V, dtype="f16", topk=300, precision=26, temp=0.9), max_batch=B)
    legs["arithmetic_topk300"] = EncodeSession(arith, bits, max_tokens=4 * a.steps)

    times = {k: [] for k in legs}
    for run in range(3):
        for name, sess in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                sess.step(logits)
            e1.record()
            e1.synchronize()
            if run > 0:
                times[name].append(1000.0 * e0.elapsed_time(e1) / a.steps)
    records = []
    for name, sess in legs.items():
        f = sess.fields()
        rec = {"leg": name, "batch": B, "vocab": V, "dtype": "f16", "steps_per_run": a.steps,
               "us_per_step": [round(t, 2) for t in times[name]],
               "bits_per_token": round(float(f["bit_pos"].sum()) / max(1, int(f["ntokens"].sum())), 3),
               "error_streams": int((f["flags"] & 6 != 0).sum())}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
