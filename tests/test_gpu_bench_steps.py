"""GPU: bench.py's headline (``lockstep_steps``) at a small batch.

* ``--steps`` sets the number of timed steps and the dumped tokens are what the product path
  (``HipArithmeticLM.encode_batch``, the slot scheduler) emits for the same streams: the first warm-up + timed tokens
  of every stream, token for token (integers: no tolerance);
* two runs with the same arguments give identical outputs;
* a run split into several passes (``EPOCH_STEPS`` lowered) still times exactly ``--steps`` steps, and its last pass
  is the next payloads' first tokens.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402
from neuralsteganography_amd import synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

B = 5  # odd, small-batch coder form; GPT-2-small geometry (the native decode step needs head_dim 64)


def _args(steps, warmup):
    return bench.parse(["--steps", str(steps), "--warmup", str(warmup), "--e2e-payload-bytes", "64",
                        "--dump-outputs", "unused"])


def _product_tokens(args, first_stream, n):
    """The first ``n`` tokens of streams ``first_stream ..`` from the provider's own batched encode."""
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    lm = HipArithmeticLM(random_gpt2(args.e2e_model), None, device="cuda:0", logits_dtype=args.e2e_logits, max_batch=B)
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(first_stream + s, 64)) for s in range(B)]
    context = [lm.vocab - 1] + list(synthetic.DEFAULT_CONTEXT[1:])
    toks = lm.encode_batch(bits, context, quality={"temp": args.temp, "precision": args.precision, "topk": args.topk})
    assert min(len(t) for t in toks) >= n
    return np.asarray([t[:n] for t in toks], dtype=np.float32)


def test_steps_are_counted_and_tokens_match_the_product_path_and_repeat():
    args = _args(4, 2)
    dev = torch.device("cuda", 0)
    run, arrays = bench.lockstep_steps(args, 0, 1, dev, batch=B)
    assert run["steps"] == 4 and run["warmup"] == 2 and run["passes"] == 1
    assert run["cover_tokens"] == 4 * B  # the timed steps alone are counted
    assert run["ms_per_step"] > 0 and run["value"] == run["payload_bits"] / run["seconds"]
    assert 0 < run["payload_bits"] <= 4 * B * (args.precision - 1)
    assert arrays["tokens"].dtype == np.float32 and arrays["tokens"].shape == (B, 6)  # 1 first + 1 warm-up + 4 timed
    assert arrays["token_rows"].tolist() == list(range(B))
    assert arrays["next_logits"].shape == (B, 50257) and np.isfinite(arrays["next_logits"]).all()
    assert (arrays["payload_bits_consumed"] <= 6 * (args.precision - 1)).all()
    assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_LIMIT
    assert np.array_equal(arrays["tokens"], _product_tokens(args, 0, 6))
    _, again = bench.lockstep_steps(args, 0, 1, dev, batch=B)
    assert sorted(again) == sorted(arrays)
    for name in arrays:
        assert np.array_equal(again[name], arrays[name]), name


def test_passes_split_the_timed_steps_exactly(monkeypatch):
    monkeypatch.setattr(bench, "EPOCH_STEPS", 4)
    args = _args(7, 2)
    run, arrays = bench.lockstep_steps(args, 0, 1, torch.device("cuda", 0), batch=B)
    # passes of (first step, untimed, timed): (1, 1, 2), (1, 0, 3), (1, 0, 2)
    assert run["steps"] == 7 and run["passes"] == 3 and run["cover_tokens"] == 7 * B
    assert arrays["tokens"].shape == (B, 3)
    assert np.array_equal(arrays["tokens"], _product_tokens(args, 2 * B, 3))  # the third pass: streams 2B .. 3B - 1
