"""GPU: the drop-in provider end to end (batched GPT-2 on PyTorch-ROCm + HIP coder).

Coder parity inside the LM loop: the logits of every step are captured and the CPU oracle replays the
coder on them; tokens must be identical.  LM parity: GPU forward vs the Hugging Face fp32 forward on CPU,
tolerance stated per compute dtype (fp32: 2e-4, fp16: 3e-2 absolute on random-init logits)."""

import numpy as np
import pytest
import torch

from neuralsteganography_amd import synthetic
from neuralsteganography_amd.codec import api as codec_api
from oracle import oracle

pytestmark = pytest.mark.gpu


def _tiny_provider(logits_dtype="f32", compute_dtype=torch.float32, seed=11, scale=1.0):
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    m = random_gpt2("tiny", vocab_size=2000, n_positions=64, seed=seed)
    # head scale 1: flat enough that no stream hits the reference coder's stall (see the stall test);
    # peaked random LMs (x2, x3) stall often, and which stream stalls depends on last-ulp logits
    with torch.no_grad():
        m.transformer.wte.weight.mul_(scale)
    return m, HipArithmeticLM(m, None, logits_dtype=logits_dtype, compute_dtype=compute_dtype)


@pytest.mark.parametrize("compute_dtype,tol", [(torch.float32, 2e-4), (torch.float16, 3e-2)])
def test_lm_logits_match_hf_within_tolerance(compute_dtype, tol):
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2

    m = random_gpt2("gpt2", seed=3)
    g = BatchedGPT2(m, device="cuda", compute_dtype=compute_dtype)
    ctx = synthetic.DEFAULT_CONTEXT
    lg = g.prefill(ctx, 2, 8)
    with torch.no_grad():
        ref = m(torch.tensor([ctx])).logits[0, -1]
    diff = (lg[0, :50257].float().cpu() - ref).abs().max().item()
    assert diff < tol, diff


def test_provider_roundtrip_and_oracle_parity():
    m, lm = _tiny_provider()
    quality = {"temp": 0.9, "precision": 26, "topk": 300}
    payloads = [synthetic.payload_bytes(s, 24) for s in range(4)]
    bits = [synthetic.bytes_to_bits_lsb(p) for p in payloads]
    context = lm.encode_seed("synthetic seed")
    # capture the logits the coder sees
    seen = []
    orig_step, orig_prefill = lm.lm.step, lm.lm.prefill

    def rec_prefill(*a, **k):
        out = orig_prefill(*a, **k)
        seen.append(out.float().cpu().numpy().copy())
        return out

    def rec_step(tok):
        out = orig_step(tok)
        seen.append(out.float().cpu().numpy().copy())
        return out

    lm.lm.prefill, lm.lm.step = rec_prefill, rec_step
    toks = lm.encode_batch(bits, context, quality=quality)
    lm.lm.prefill, lm.lm.step = orig_prefill, orig_step
    V = lm.vocab
    for s in range(4):
        o, _ = oracle.encode_stream(lambda t: seen[t][s, :V], bits[s], banned=[V - 1, 628], temp=0.9,
                                    precision=26, topk=300)
        assert o == toks[s], f"stream {s}: coder inside the LM loop differs from the oracle"
    out = lm.decode_batch(toks, context, quality=quality)
    for s in range(4):
        assert out[s][: len(bits[s])] == bits[s]


def test_codec_slot_roundtrip_through_provider():
    _, lm = _tiny_provider()
    quality = {"temp": 1.0, "precision": 20, "topk": 200}
    msg = b"payload via codec.api"
    toks = codec_api.encode_arithmetic(msg, lm, quality=quality, seed_text="ctx")
    assert codec_api.decode_arithmetic(toks, lm, quality=quality, seed_text="ctx") == msg


def test_state_side_channel_like_reference_envelope():
    """drain_states/load_states carry the bit count (CodecState residual_bits) as api.encode_text expects."""
    _, lm = _tiny_provider()
    quality = {"temp": 1.0, "precision": 16, "topk": 100}
    bits = synthetic.bytes_to_bits_lsb(b"\x01\x02\x03")
    ctx = lm.encode_seed("")
    toks = lm.encode_arithmetic(bits, ctx, quality=quality)
    states = lm.drain_states()
    assert len(states) == 1 and int.from_bytes(states[0]["residual_bits"], "big") == 24
    lm.load_states(states)
    assert lm.decode_arithmetic(toks, ctx, quality=quality) == bits


def test_reference_stall_is_reported_not_hung():
    """A dominant token fixes no bit: q_0 = R every step, the interval never shrinks, and the reference
    coder's ``while i < len(message)`` (code_base/arithmetic.py:114) would spin forever.  The provider
    reports it after ``stall_steps`` tokens.  The LM boundary returns rows where token 5 dominates."""
    from neuralsteganography_amd.codec.errors import ArithmeticRangeError

    _, lm = _tiny_provider()
    ld = lm.lm.ld

    def dominant(B):
        row = torch.zeros((B, ld), device="cuda", dtype=torch.float32)
        row[:, 5] = 80.0
        return row

    lm.lm.prefill = lambda ctx, B, n: (setattr(lm.lm, "B", B), dominant(B))[1]
    lm.lm.step = lambda tok: dominant(tok.shape[0])
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 4)) for s in range(2)]
    with pytest.raises(ArithmeticRangeError):
        lm.encode_batch(bits, [1999], quality={"temp": 1.0, "precision": 26, "topk": 300}, stall_steps=64)


def test_provider_finish_sent_matches_oracle():
    """quality['finish_sent'] (code_base/arithmetic.py:114,134-137): the LM loop keeps emitting top-1 tokens
    after the payload until a sentence-ending one; the coder's choices inside the loop equal the oracle's
    replay on the captured logits, and decode recovers the payload from the longer cover."""
    _, lm = _tiny_provider()
    V = lm.vocab
    # random tied-embedding LMs fall into greedy fixed points, so the table marks most ids (tails stay short);
    # long tails are covered on synthetic rows in test_gpu_parity.test_finish_sent_matches_oracle
    table = (np.arange(V) % 8 != 3).astype(np.uint8)
    lm._sent_end = table
    quality = {"temp": 0.9, "precision": 26, "topk": 300, "finish_sent": True}
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 6))[: [48, 5, 0][s]] for s in range(3)]
    context = lm.encode_seed("finish")
    seen = []
    orig_step, orig_prefill = lm.lm.step, lm.lm.prefill

    def rec_prefill(*a, **k):
        out = orig_prefill(*a, **k)
        seen.append(out.float().cpu().numpy().copy())
        return out

    def rec_step(tok):
        out = orig_step(tok)
        seen.append(out.float().cpu().numpy().copy())
        return out

    lm.lm.prefill, lm.lm.step = rec_prefill, rec_step
    toks = lm.encode_batch(bits, context, quality=quality, stall_steps=512)
    lm.lm.prefill, lm.lm.step = orig_prefill, orig_step
    for s in range(3):
        o, _ = oracle.encode_stream(lambda t: seen[t][s, :V], bits[s], banned=[V - 1, 628], temp=0.9,
                                    precision=26, topk=300, sent_end=table)
        assert o == toks[s], f"stream {s}: finish_sent inside the LM loop differs from the oracle"
        assert table[toks[s][-1]]
    out = lm.decode_batch([t for t in toks if t], context, quality=quality)
    for b, got in zip([b for b, t in zip(bits, toks) if t], out):
        assert got[: len(b)] == b


def test_provider_finish_sent_without_sentence_end_is_reported():
    """No id ends a sentence: the reference would generate forever; the provider raises after stall_steps."""
    from neuralsteganography_amd.codec.errors import ArithmeticRangeError

    _, lm = _tiny_provider()
    lm._sent_end = np.zeros(lm.vocab, dtype=np.uint8)
    bits = [synthetic.bytes_to_bits_lsb(b"\x05")]
    with pytest.raises(ArithmeticRangeError, match="finish_sent"):
        lm.encode_batch(bits, lm.encode_seed(""), quality={"temp": 1.0, "precision": 20, "topk": 100,
                                                            "finish_sent": True}, stall_steps=64)


def test_batched_front_end_multi_message_roundtrip():
    """stego_encode_batch / stego_decode_batch (api.py:707-807 batched): every packet of every message is a
    stream of one lockstep GPT-2 + HIP-coder loop; RS + CRC framing; decode needs no state side channel."""
    from neuralsteganography_amd.stego import stego_decode_batch, stego_encode_batch

    _, lm = _tiny_provider()
    msgs = [synthetic.payload_bytes(s, n) for s, n in enumerate((1, 40, 130, 0))]
    q = {"temp": 1.0, "precision": 16, "topk": 300, "finish_sent": False}
    res = stego_encode_batch(msgs, chunk_bytes=64, quality=q, seed_text="seed", lm=lm)
    assert [r.metadata.total for r in res] == [1, 1, 3, 1]
    lm.load_states([])  # decode must not depend on the bit-count side channel
    assert stego_decode_batch([list(r) for r in res], quality=q, seed_text="seed", lm=lm) == msgs


@pytest.mark.parametrize("B,H,L0", [(3, 12, 0), (3, 12, 1), (5, 12, 7), (4, 16, 8), (2, 12, 33), (7, 12, 200),
                                    # the rows of a pair are split over waves by its KEY COUNT L0 + 1 alone
                                    # (<= 256: 1 wave, <= 512: 2, <= 1024: 4, above: 8), whatever the batch:
                                    (2, 16, 1023), (1, 12, 500),  # 1,024 keys: 4 waves; 501 keys: 2 waves
                                    (40, 12, 77), (64, 16, 3),    # 1 wave; <= 1024 pairs: one pair per workgroup
                                    (100, 12, 50)])               # 1 wave; 1,200 pairs: eight pairs per workgroup
def test_hip_decode_attention_matches_fp32_reference(B, H, L0):
    """ns_decode_attention (csrc/nsg_attn.hip) vs softmax(q k^T / sqrt(D)) v in fp32 (torch) over the cache
    plus the appended token; the kernel must also have written the new k/v at position L0.  fp16 output:
    2e-3 absolute on O(1) values."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import _stream_handle

    D, cap = 64, L0 + 5
    g = torch.Generator(device="cuda").manual_seed(100 + L0)
    qkv = torch.randn((B, 3 * H * D), generator=g, device="cuda").half()
    kc = torch.randn((B, H, cap, D), generator=g, device="cuda").half()
    vc = torch.randn((B, H, cap, D), generator=g, device="cuda").half()
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B, H * D), float("nan"), device="cuda").half()
    rc = _lib.lib().ns_decode_attention(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0),
                                        kc.stride(1), B, H, D, L0, out.data_ptr(), out.stride(0), D ** -0.5,
                                        _stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    q, k, v = qkv.view(B, 3, H, D).float().unbind(1)
    kk = kc0.float().clone()
    vv = vc0.float().clone()
    kk[:, :, L0] = k
    vv[:, :, L0] = v
    s = torch.einsum("bhd,bhjd->bhj", q, kk[:, :, : L0 + 1]) * D ** -0.5
    want = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), vv[:, :, : L0 + 1]).reshape(B, H * D)
    assert (out.float() - want).abs().max().item() < 2e-3
    assert torch.equal(kc[:, :, L0], k.half()) and torch.equal(vc[:, :, L0], v.half())
    assert torch.equal(kc[:, :, :L0], kc0[:, :, :L0]) and torch.equal(kc[:, :, L0 + 1:], kc0[:, :, L0 + 1:])


def test_hip_decode_attention_rejects_bad_shapes():
    from neuralsteganography_amd import _lib

    t = torch.zeros((2, 3 * 64), device="cuda").half()
    c = torch.zeros((2, 1, 4, 64), device="cuda").half()
    f = _lib.lib().ns_decode_attention
    assert f(t.data_ptr(), t.stride(0), c.data_ptr(), c.data_ptr(), c.stride(0), c.stride(1), 2, 1, 32, 0,
             t.data_ptr(), 64, 0.1, None) == _lib.NS_ERR_UNSUPPORTED  # head_dim 32
    assert f(t.data_ptr(), t.stride(0), c.data_ptr(), c.data_ptr(), c.stride(0), c.stride(1), 2, 1, 64, 4,
             t.data_ptr(), 64, 0.1, None) == _lib.NS_ERR_CONFIG  # L0 beyond the cache capacity


@pytest.mark.parametrize("B", [3, 1])
def test_gpt2_fp16_decode_hip_attention_matches_sdpa_and_hf(B):
    """GPT-2-small fp16 decode steps: the native HIP step (nsg_lm GEMMs / layer norms + HIP attention) vs the
    PyTorch path on identical weights (fp16 round-off only), and the last step vs Hugging Face fp32 on CPU over
    the whole sequence (3e-2 absolute)."""
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2

    m = random_gpt2("gpt2", seed=5)
    a = BatchedGPT2(m, device="cuda", compute_dtype=torch.float16)
    b = BatchedGPT2(m, device="cuda", compute_dtype=torch.float16)
    b.native = False  # the PyTorch decode path (hipBLASLt GEMMs + SDPA) on the same weights
    assert a.native
    ctx = synthetic.DEFAULT_CONTEXT
    la, lb = a.prefill(ctx, B, 4), b.prefill(ctx, B, 4)
    toks = [[11, 500, 9000], [7, 7, 7], [42, 43, 44], [50000, 1, 2], [3, 4, 5], [9, 8, 7]]
    toks = [t[-B:] for t in toks]
    for t in toks:  # 6 steps: past the initial 4-position budget, so the cache grows once
        tt = torch.tensor(t, device="cuda")
        la, lb = a.step(tt), b.step(tt)
        assert (la.float() - lb.float()).abs().max().item() < 2e-2
    row = min(1, B - 1)
    seq = list(ctx) + [t[row] for t in toks]
    with torch.no_grad():
        ref = m(torch.tensor([seq])).logits[0, -1]
    assert (la[row, :50257].float().cpu() - ref).abs().max().item() < 3e-2


@pytest.mark.parametrize("cap_pages,topk,n", [(None, 300, 3), (3, 300, 3), (None, 50000, 3), (None, 300, 1)])
def test_graph_captured_encode_matches_eager(cap_pages, topk, n):
    """encode_batch with the per-token step captured as a hipGraph (coder + GPT-2 decode, cache lengths on the
    device) gives the same tokens as the eager loop, including when the page pool is capped (cap_pages: the
    youngest streams are re-queued, the graph re-captured), and for the api default quality (precision 16, topk
    50,000), whose wide-path launches (memset, fused scan, device-wide sort, list kernel) are captured too."""
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    m = random_gpt2("gpt2", seed=31)
    q = {"temp": 0.9, "precision": 26, "topk": 300} if topk == 300 else {"temp": 1.0, "precision": 16,
                                                                        "topk": topk}
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 12)) for s in range(n)]
    ctx = synthetic.DEFAULT_CONTEXT
    out = {}
    for graphs in (False, True):
        lm = HipArithmeticLM(m, None, logits_dtype="f16")
        if cap_pages is not None:
            lm.lm.kv_segment_pages = 1  # a page-exact budget
            pool = lm.lm.page_pool()
            pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
        out[graphs] = lm.encode_batch(bits, ctx, quality=q, graphs=graphs)
        dec = lm.decode_batch(out[graphs], ctx, quality=q, graphs=graphs)
        assert all(d[: len(b)] == b for d, b in zip(dec, bits))
        out[("dec", graphs)] = dec
    assert out[True] == out[False] and out[("dec", True)] == out[("dec", False)]


def test_coder_context_cache_reuses_and_bounds():
    """coder contexts are keyed on the parameters only -- a context built for a larger batch
    serves smaller ones, a larger batch replaces it, and at most CTX_CACHE_SIZE parameter sets stay alive."""
    from neuralsteganography_amd.coder import CoderParams
    from neuralsteganography_amd.lm import arithmetic as arith

    _, lm = _tiny_provider()
    p = CoderParams(vocab=lm.vocab, precision=26, temp=0.9, topk=300, dtype="f32")
    c8 = lm._coder(p, 8)
    assert lm._coder(p, 3) is c8 and c8.max_batch == 8  # smaller batch: same context
    c16 = lm._coder(p, 16)
    assert c16 is not c8 and c16.max_batch == 16 and c8._h is None  # replaced and closed
    for t in range(arith.CTX_CACHE_SIZE + 2):  # distinct parameter sets: LRU-bounded
        lm._coder(CoderParams(vocab=lm.vocab, precision=26, temp=0.5 + 0.1 * t, topk=300, dtype="f32"), 4)
    assert len(lm._ctx_cache) == arith.CTX_CACHE_SIZE
    assert c16._h is None  # the oldest one was evicted and closed


def test_stop_text_stops_inside_graph_replay():
    """the '<eos>' stop of the code_base entry points runs with the hipGraph-captured step (a
    device table of ids that can complete the stop text + one flag per token); the stopped stream's tokens end
    with the stop text, as the reference's decoded-text check stops (code_base/arithmetic.py:207-210)."""
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    class TwoCharTok:
        """ids < 256: a byte; id 300: '<eos>' as one token (so the stop fires exactly when it is emitted)."""

        def decode(self, ids):
            return "".join("<eos>" if int(i) == 300 else chr(int(i) % 256) for i in ids)

        def encode(self, text, add_special_tokens=False):
            return [ord(ch) for ch in text]

    m = random_gpt2("tiny", vocab_size=512, n_positions=512, n_embd=128, n_head=2, seed=3)
    lm = HipArithmeticLM(m, TwoCharTok(), compute_dtype=torch.float16, logits_dtype="f32")
    # a wide temperature flattens the random LM so id 300 shows up within a few hundred tokens for some streams
    q = {"temp": 3.0, "precision": 26, "topk": 500}
    bits = [synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(s, 384)) for s in range(8)]
    toks_g = lm.encode_batch(bits, [1, 2, 3], quality=q, stop_text="<eos>", graphs=True)
    toks_e = lm.encode_batch(bits, [1, 2, 3], quality=q, stop_text="<eos>", graphs=False)
    assert toks_g == toks_e
    stopped = [t for t in toks_g if 300 in t]
    assert stopped, "no stream emitted the stop token: pick another seed"
    for t in stopped:
        assert t[-1] == 300 and t.count(300) == 1  # stops right after the first '<eos>'
