"""Paged decode attention at short key counts: fixed cost per launch and cost per own row.

    python tools/paged_short_probe.py [--tag NAME] [--out FILE.jsonl]

Sibling of ``paged_attn_probe.py`` (layout (c): layer-major segments, pages in allocation order).  B = 4,096 streams on
a shared 32-token context, every stream at the same length L; L in {32, 40, 64, 96, 160, 250} (1-219 own rows, one
wave per pair) for fp16 and for fp8 with window 256, then L = 544 and 900 (fp16, split pairs: the general path) and
B = 1 at L = 250 and 900 (one pair per workgroup).  Successive launches walk the layers of a 12-layer pool, as a
decode step does, so a launch does not find its own rows from the launch before in the cache.  Prints one JSON
line per point (average kernel time over the launches, HIP events) and one per fit: kernel_us = fixed_us +
per_row_us * own_rows, least squares over the six short lengths.  Compare two builds of the library by running the
tool once per build (``NSG_CODER_LIB``), alternating.
"""

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.coder import _stream_handle  # noqa: E402

H, D, T0 = 12, 64, 32
SHORT = (32, 40, 64, 96, 160, 250)


def measure(B, L, kv, window, layers, steps):
    C = H * D
    nch = (L + 1 - T0 + 31) // 32
    edt = torch.uint8 if kv == "fp8" else torch.float16
    fmt = _lib.NS_KV_FP8 if kv == "fp8" else _lib.NS_KV_FP16
    esz = 1 if kv == "fp8" else 2
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv = torch.randn((B, 3 * C), generator=g, device="cuda", dtype=torch.float16)
    kp = torch.zeros((H, T0, D), device="cuda", dtype=edt)
    vp = torch.zeros((H, T0, D), device="cuda", dtype=edt)
    out = torch.empty((B, C), device="cuda", dtype=torch.float16)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    npages = B * nch
    blk = 2 * H * 32 * D  # one layer's block of a page, elements
    pool = torch.zeros((layers, npages, blk), device="cuda", dtype=edt)
    order = np.arange(npages).reshape(nch, B).T  # page of (stream b, chunk c) = c * B + b
    table = torch.from_numpy(np.ascontiguousarray(pool.data_ptr() + blk * esz * order.astype(np.int64))).cuda()
    lib, st = _lib.lib(), _stream_handle()

    def launch(i):
        rc = lib.ns_decode_attention_paged(qkv.data_ptr(), qkv.stride(0), table.data_ptr(), table.stride(0),
                                           table.shape[1], (i % layers) * npages * blk, kp.data_ptr(), vp.data_ptr(),
                                           kp.stride(0), T0, B, H, D, lens.data_ptr(), window, fmt, None, 0, None,
                                           out.data_ptr(), out.stride(0), 1.0 / math.sqrt(D), st)
        assert rc == 0, rc

    for i in range(layers):
        launch(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--steps", type=int, default=120)
    a = ap.parse_args()
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        rec = {"tag": a.tag, "lib": _lib.version(), **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for kv, window in (("fp16", 0), ("fp8", 256)):
        xs, ys = [], []
        for L in SHORT:
            us = measure(4096, L, kv, window, 12, a.steps)
            own = L + 1 - T0
            xs.append(own)
            ys.append(us)
            emit({"B": 4096, "L": L, "kv": kv, "window": window, "own_rows": own, "kernel_us": us})
        per_row, fixed = np.polyfit(np.array(xs, dtype=np.float64), np.array(ys), 1)
        emit({"B": 4096, "kv": kv, "window": window, "fit": "kernel_us = fixed_us + per_row_us * own_rows",
              "fixed_us": float(fixed), "per_row_us": float(per_row)})
    for L in (544, 900):
        emit({"B": 4096, "L": L, "kv": "fp16", "window": 0, "own_rows": L + 1 - T0,
              "kernel_us": measure(4096, L, "fp16", 0, 2, max(a.steps // 4, 12))})
    for L in (250, 900):
        emit({"B": 1, "L": L, "kv": "fp16", "window": 0, "own_rows": L + 1 - T0,
              "kernel_us": measure(1, L, "fp16", 0, 12, 4 * a.steps)})


if __name__ == "__main__":
    main()
