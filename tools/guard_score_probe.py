"""The guard's scoring forward, padded against packed against the fused head; cover generation with one seed per
message, one batched call against one call per seed.

    python tools/guard_score_probe.py score [--texts 1024] [--min-tokens 100] [--max-tokens 1000]
                                            [--legs padded,packed,fused] [--repeats 2] [--out FILE]
    python tools/guard_score_probe.py cover [--secrets 256] [--payload-bytes 32] [--legs batch,per_seed]
                                            [--repeats 2] [--out FILE]

GPT-2-small (random weights, fp16 native path).  Legs run alternating ``--repeats`` times after one untimed pass of
each; one JSON line per leg.

``score``: ``--texts`` texts of ``--min-tokens`` to ``--max-tokens`` byte tokens through ``HipLMScorer.metrics_batch``
(fp32 logits, the default ``rows_per_batch``): ``padded`` (``packed=False``), ``packed`` (the default) and ``fused``
(``packed=True, fused_head=True``).  Per leg: the wall seconds of every repeat, the rows run against the texts' own rows,
``torch.cuda.max_memory_allocated`` over the leg's timed repeats and a SHA-256 of all metrics (``padded`` and ``packed``
must agree; ``fused`` differs in the last bits).  On a checkout whose scorer has no ``packed`` switch the tool runs the one
leg it can, ``base``, so the same file measures the parent commit.

``cover``: ``--secrets`` secrets with as many distinct seeds, gate on with the GPU guard, ``max_ppl`` at the median
perplexity of the attempt-1 covers (found in an untimed pass through ``stego_encode_batch(seed_texts=...)``, the same
code in both builds) so that about half the messages go on to the pool seeds: ``batch``, one
``cover_generate_batch(seed_texts=...)`` call, against ``per_seed``, one ``cover_generate_batch([s], seed_text=...)`` call
per message (the only form the parent commit has).  The untimed pass of ``per_seed`` covers the first 8 messages only.
Per leg: wall seconds, how many covers passed and a SHA-256 of all texts (a rejected message: its last attempt's text).
"""

import argparse
import hashlib
import inspect
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from neuralsteganography_amd import _lib  # noqa: E402
from neuralsteganography_amd.lm.arithmetic import ByteTokenizer, HipArithmeticLM  # noqa: E402
from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2  # noqa: E402
from neuralsteganography_amd.metrics import HipLMScorer, LMScorer  # noqa: E402

Q = {"temp": 0.9, "precision": 26, "topk": 300, "finish_sent": False}
OPEN_GATE = {"max_ppl": 1e12, "max_ngram_repeat": 1.0, "min_ttr": 0.0, "max_avg_entropy": 1e9}


def padded_rows(lens, rows_per_batch):
    """Rows the padded path runs for texts of ``lens`` tokens (the grouping of ``HipLMScorer._row_scores``)."""
    lens = sorted(lens)
    i = rows = 0
    while i < len(lens):
        j = i
        while j < len(lens) and (j - i + 1) * lens[j] <= max(rows_per_batch, lens[i]):
            j += 1
        rows += (j - i) * lens[j - 1]
        i = j
    return rows


def digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def score(a, emit):
    lm = BatchedGPT2(random_gpt2("gpt2", seed=7), device="cuda", compute_dtype=torch.float16,
                     logits_dtype=torch.float32)
    tok = ByteTokenizer(50257)
    rng = np.random.default_rng(2026)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz    "))
    texts = []
    for _ in range(a.texts):
        t = "".join(rng.choice(letters, size=int(rng.integers(a.min_tokens, a.max_tokens + 1))))
        texts.append("x" + t[1:-1] + "x")  # no leading / trailing blank: the byte count is the token count
    lens = [len(t) for t in texts]
    has_switch = "packed" in inspect.signature(HipLMScorer.__init__).parameters
    legs = a.legs.split(",") if has_switch else ["base"]
    kws = {"base": {}, "padded": {"packed": False}, "packed": {"packed": True},
           "fused": {"packed": True, "fused_head": True}}
    scorers = {leg: HipLMScorer(lm, tok, **kws[leg]) for leg in legs}

    def run(leg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = scorers[leg].metrics_batch(texts)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for leg in legs:
        run(leg)
    walls = {leg: [] for leg in legs}
    peak = {leg: 0 for leg in legs}
    res = {}
    for _ in range(a.repeats):
        for leg in legs:
            torch.cuda.reset_peak_memory_stats()
            res[leg], w = run(leg)
            walls[leg].append(round(w, 4))
            peak[leg] = max(peak[leg], int(torch.cuda.max_memory_allocated()))
    for leg in legs:
        rows = getattr(scorers[leg], "last_rows", None)
        run_rows = rows["rows"] if rows else padded_rows(lens, scorers[leg].rows_per_batch)
        emit({"leg": leg, "wall_s": walls[leg], "rows_run": int(run_rows), "rows_real": int(sum(lens)),
              "max_memory_allocated": peak[leg], "metrics_sha256": digest(res[leg])})
    if "padded" in res and "packed" in res:
        same = digest(res["padded"]) == digest(res["packed"])
        emit({"leg": "check", "packed_equals_padded": same})
        assert same, "packed and padded disagree on a text's metrics"
    if "fused" in res and "packed" in res:
        d = max(abs(f[k] - p[k]) / (abs(p[k]) + 1.0) for f, p in zip(res["fused"], res["packed"])
                for k in ("avg_nll", "avg_entropy"))
        emit({"leg": "check", "fused_vs_packed_max_rel": d})


def cover(a, emit):
    from neuralsteganography_amd import stego, synthetic
    from neuralsteganography_amd.codec.textio import seed_to_ids, spans_to_text
    from neuralsteganography_amd.cover import cover_generate_batch
    from neuralsteganography_amd.detect import QualityGuard

    stego.make_msg_id = lambda: "00000000-0000-4000-8000-000000000001"  # the same packets in every leg and build
    lm = HipArithmeticLM(random_gpt2("gpt2", seed=7), None, logits_dtype="f16", logit_scale=a.scale)
    guard = QualityGuard(lm_scorer=LMScorer(scorer=HipLMScorer.from_provider(lm)))
    rng = np.random.default_rng(2026)
    words = ["alpha", "beta", "gamma", "delta", "stego", "cover", "token", "text", "seed", "talk"]
    N = a.secrets
    seeds = [f"conversation {i}: " + " ".join(rng.choice(words, size=int(rng.integers(4, 12)))) + ". " for i in range(N)]
    secrets = [synthetic.payload_bytes(7000 + s, a.payload_bytes) for s in range(N)]
    # untimed: the attempt-1 covers of every message, for the threshold
    res = stego.stego_encode_batch(secrets, quality=Q, seed_texts=seeds, lm=lm)
    first = [spans_to_text([list(map(int, s)) for s in r], seed_to_ids(seed, lm.tokenizer), lm.tokenizer)
             for r, seed in zip(res, seeds)]
    ppl = sorted(v.metrics["ppl"] for v in guard.evaluate_batch(first, OPEN_GATE))
    gate = dict(OPEN_GATE, max_ppl=float(ppl[N // 2]))
    kw = dict(quality=Q, lm=lm, quality_guard=guard, gate_thresholds=gate, return_errors=True)
    has_seeds = "seed_texts" in inspect.signature(cover_generate_batch).parameters
    legs = [leg for leg in a.legs.split(",") if has_seeds or leg == "per_seed"]

    def run(leg, n=N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "batch":
            out = cover_generate_batch(secrets[:n], seed_texts=seeds[:n], **kw)
        else:
            out = [cover_generate_batch([s], seed_text=seed, **kw)[0] for s, seed in zip(secrets[:n], seeds[:n])]
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for leg in legs:
        run(leg, N if leg == "batch" else min(N, 8))
    walls = {leg: [] for leg in legs}
    out = {}
    for _ in range(a.repeats):
        for leg in legs:
            out[leg], w = run(leg)
            walls[leg].append(round(w, 3))
    for leg in legs:
        texts = [o if isinstance(o, str) else o.cover_text for o in out[leg]]
        emit({"leg": leg, "wall_s": walls[leg], "secrets": N, "passed": sum(isinstance(o, str) for o in out[leg]),
              "max_ppl": gate["max_ppl"], "texts_sha256": digest(texts)})
    if len(legs) == 2:
        same = [_plain(o) for o in out[legs[0]]] == [_plain(o) for o in out[legs[1]]]
        emit({"leg": "check", "same_texts": same})
        assert same, "the batched call and the per-seed calls disagree on a cover"


def _plain(o):
    return o if isinstance(o, str) else ("rejected", o.cover_text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["score", "cover"])
    ap.add_argument("--texts", type=int, default=1024)
    ap.add_argument("--min-tokens", type=int, default=100)
    ap.add_argument("--max-tokens", type=int, default=1000)
    ap.add_argument("--secrets", type=int, default=256)
    ap.add_argument("--payload-bytes", type=int, default=32)
    ap.add_argument("--scale", type=float, default=6.0, help="head scale (6: trained-LM-like rows, ~4 bits per token)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.legs is None:
        a.legs = "padded,packed,fused" if a.mode == "score" else "batch,per_seed"
    base = {"tool": "guard_score_probe", "mode": a.mode, "library": _lib.version(),
            "device": torch.cuda.get_device_name(0)}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    (score if a.mode == "score" else cover)(a, emit)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
