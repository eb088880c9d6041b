"""GPU: ``BatchedGPT2.step_chunk`` / ``step_chunk_static`` (C known tokens per stream in one forward) against ``step``
fed one token at a time: every logits row, ``kv.lens`` and every byte of the KV pages must be the same bits.

A tiny native GPT-2 (n_embd 128, 2 heads, 2 layers, n_positions 64, vocab 512), three streams with different context
lengths, C = 5 from position ~50 to past 140: the position embedding wraps twice and chunks cross page boundaries.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

C = 5
CTX_LENS = [50, 53, 61]
NTOK = 92  # 50 + 92 = 142 > 140; not a multiple of C
V = 512


def _model():
    from neuralsteganography_amd.lm.gpt2 import BatchedGPT2, random_gpt2

    hf = random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=V, n_positions=64)
    lm = BatchedGPT2(hf, device="cuda", compute_dtype=torch.float16, logits_dtype=torch.float16)
    assert lm.native
    return lm


def _start(lm, contexts, ahead=NTOK + 1):
    """A fresh call with every page of the run mapped up front -- the same pages in the same order whichever way the
    tokens are then fed -- and the pool zeroed, so pages written by an earlier run cannot pass for this one's."""
    B = len(contexts)
    lm.begin_slots(B, 0, 256)
    slots = np.arange(B)
    tl = np.asarray([len(c) for c in contexts], dtype=np.int64)
    assert lm.kv.ensure(slots, tl + ahead).size == 0
    for seg in lm.pool.segments:
        seg.zero_()
    return lm.prefill_contexts(contexts, slots)


def _pages(lm):
    """Every byte of the pool and the page table (the same addresses in every run of :func:`_start`)."""
    torch.cuda.synchronize()
    return [seg.clone() for seg in lm.pool.segments] + [lm.kv.table.clone()]


@pytest.fixture(scope="module")
def reference():
    """The one-token run, computed once: logits per step, final lengths and pages."""
    rng = np.random.default_rng(5)
    contexts = [rng.integers(0, V, size=n).tolist() for n in CTX_LENS]
    toks = rng.integers(0, V, size=(len(CTX_LENS), NTOK)).astype(np.int32)
    lm = _model()
    _start(lm, contexts)
    rows = []
    for t in range(NTOK):
        rows.append(lm.step(torch.from_numpy(toks[:, t]).cuda()).clone())
    ref = torch.stack(rows, dim=1)  # [B, NTOK, ld]
    lens = lm.kv.lens.cpu().numpy().copy()
    return lm, contexts, toks, ref, lens, _pages(lm)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_step_chunk_equals_step_one_token_at_a_time(reference):
    lm, contexts, toks, ref, lens_ref, pages_ref = reference
    assert torch.isfinite(ref.float()).all()
    B = len(contexts)
    _start(lm, contexts)
    for t0 in range(0, NTOK, C):
        n = min(C, NTOK - t0)
        chunk = np.zeros((B, C), dtype=np.int32)
        chunk[:, :n] = toks[:, t0: t0 + n]
        out = lm.step_chunk(torch.from_numpy(chunk).cuda(), [n] * B)
        assert out.shape == (B, C, lm.ld)
        assert _same_bits(out[:, :n], ref[:, t0: t0 + n]), t0
    assert np.array_equal(lm.kv.lens.cpu().numpy(), lens_ref)
    assert np.array_equal(lm.kv.lens_host, lens_ref)
    for b, (p, q) in enumerate(zip(_pages(lm), pages_ref)):
        assert torch.equal(p, q), b


def test_step_chunk_static_under_graph_replay_with_streams_ending_mid_chunk(reference):
    """Three replays of one captured ``step_chunk_static``; the counts (device memory the graph reads) end stream 0
    after 7 tokens and stream 2 after 11, both mid-chunk; stream 1 runs all 15."""
    lm, contexts, toks, ref, _, _ = reference
    B = len(contexts)
    total = np.asarray([7, 15, 11])
    _start(lm, contexts)
    base = lm.kv.lens_host.copy()
    logits = torch.zeros((B, C, lm.ld), device="cuda", dtype=lm.logits_dtype)
    tok_dev = torch.zeros((B, C), dtype=torch.int32, device="cuda")
    cnt_dev = torch.zeros(B, dtype=torch.int32, device="cuda")
    lm.begin_chunk_static(logits)

    def load(it):
        n = np.clip(total - it * C, 0, C)
        tok_dev.copy_(torch.from_numpy(np.ascontiguousarray(toks[:, it * C: it * C + C])).cuda())
        cnt_dev.copy_(torch.from_numpy(n.astype(np.int32)).cuda())
        return n

    def check(it, n):
        torch.cuda.synchronize()
        for b in range(B):
            assert _same_bits(logits[b, : n[b]], ref[b, it * C: it * C + n[b]]), (it, b)
        lm.advance_rows(n)
        assert np.array_equal(lm.kv.lens.cpu().numpy(), lm.kv.lens_host)

    n = load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lm.step_chunk_static(tok_dev, cnt_dev)  # iteration 0, eager (warms the kernels up)
    torch.cuda.current_stream().wait_stream(side)
    check(0, n)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lm.step_chunk_static(tok_dev, cnt_dev)
    for it in (1, 2):
        n = load(it)
        graph.replay()
        check(it, n)
    assert np.array_equal(lm.kv.lens_host, base + total)


def test_chunk_step_refuses_what_it_cannot_do(reference):
    lm = reference[0]
    B = lm.kv.B
    with pytest.raises(ValueError):
        lm.step_chunk(torch.zeros((B, 17), dtype=torch.int32, device="cuda"), [1] * B)
    with pytest.raises(ValueError):
        lm.step_chunk(torch.zeros((B, C), dtype=torch.int32, device="cuda"), [C + 1] * B)
    lm.window = 8
    try:
        with pytest.raises(ValueError):
            lm.step_chunk(torch.zeros((B, C), dtype=torch.int32, device="cuda"), [1] * B)
    finally:
        lm.window = 0
