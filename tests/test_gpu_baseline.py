"""GPU: the fixed-block baseline coders (``ns_huffman_*`` / ``ns_bins_*``, include/nsg_baseline.h) against the Python
restatement (``tests/baseline_cases.py``) token by token and bit by bit, the error and divergence contracts, every
golden of the reference through the kernels, the slot-scheduled batch on a tiny native GPT-2 and the ``code_base``
entry points."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import baseline_cases as bc

pytestmark = pytest.mark.gpu

STAT_RTOL = 2e-5  # the project's bound for statistics against the reference


def _ctx(V, dtype, B):
    from neuralsteganography_amd.coder import CoderContext, CoderParams

    return CoderContext(CoderParams(vocab=V, dtype=dtype, topk=2), max_batch=B, device=0)


def _dev(rows, ld, dtype):
    """[B, V] host rows -> [B, ld] device logits of the context's dtype (padding: large, must never be read)."""
    import torch

    B, V = rows.shape
    out = np.full((B, ld), 1.0e4, dtype=np.float16 if dtype == "f16" else np.float32)
    out[:, :V] = rows
    return torch.from_numpy(out).cuda()


@functools.lru_cache(maxsize=None)
def _rows(V, dtype, B, block, nsteps, seed=3):
    """[nsteps, B, V] rows (fp32 values; fp16-representable for "f16"): stream b % 4 == 1 has exact ties among its
    leaders (values on a coarse grid), b % 4 == 2 has its K-th and (K+1)-th values tied, b % 4 == 3 is peaked."""
    rng = np.random.default_rng(seed + 1000 * block + B)
    K = 1 << block
    x = (rng.standard_normal((nsteps, B, V)) * 2.0).astype(np.float32)
    for b in range(B):
        if b % 4 == 1:
            x[:, b] = np.round(x[:, b] * 2.0) / 2.0
        elif b % 4 == 3:
            x[:, b] *= 4.0
    if dtype == "f16":
        x = x.astype(np.float16).astype(np.float32)
    banned = [V - 1, 628]
    for b in range(2, B, 4):
        for t in range(nsteps):
            r = x[t, b]
            order = bc.ranking(r + np.float32(0), bc._banned_mask(V, banned))
            r[order[K]] = r[order[K - 1]]  # the K-th and (K+1)-th values tie: the lower id leads
    x.setflags(write=False)
    return x


def _payloads(B, block):
    lens = [0, 1, block - 1, 2 * block + 1, 19, 8 * block]
    rng = np.random.default_rng(17)
    return [rng.integers(0, 2, size=lens[b % len(lens)]).tolist() for b in range(B)]


STEP_CASES = [(700, 704, 67, blk, dt) for blk in (1, 3, 8) for dt in ("f32", "f16")] + \
             [(700, 768, 5, 3, "f32"), (700, 768, 5, 3, "f16"), (50257, 50304, 5, 3, "f32"), (50257, 50304, 5, 8, "f32"),
              (50257, 50304, 5, 3, "f16"), (50257, 50304, 5, 8, "f16"), (50257, 50304, 1, 1, "f32"),
              (50257, 50304, 67, 3, "f16")]


@pytest.mark.parametrize("mode", ["huffman", "bins"])
@pytest.mark.parametrize("V,ld,B,block,dtype", STEP_CASES)
def test_steps_equal_the_restatement(mode, V, ld, B, block, dtype):
    """Encode (tokens, bits consumed, statistics), then both decode forms (bits), stream by stream."""
    from neuralsteganography_amd.coder import (BaselineDecodeSession, BaselineDecodeStreamsSession,
                                               BaselineEncodeSession)

    banned = [V - 1, 628]
    bits = _payloads(B, block)
    R = 3  # distinct row sets, reused in turn: step t reads rows[t % R]
    rows = _rows(V, dtype, B, block, R)
    table = bc.word2bin_table(V, block) if mode == "bins" else None
    ref = []
    for b in range(B):
        fn = (lambda t, b=b: rows[t % R, b])
        if mode == "huffman":
            ref.append(bc.huffman_encode_stream(fn, bits[b], banned=banned, block_size=block))
        else:
            ref.append(bc.bins_encode_stream(fn, bits[b], banned=banned, block_size=block, table=table))
    ctx = _ctx(V, dtype, B)
    sess = BaselineEncodeSession(ctx, bits, mode=mode, block_size=block, stats=True)
    dev_rows = [_dev(rows[r], ld, dtype) for r in range(R)]
    for t in range(max(len(r[0]) for r in ref) + 1):
        sess.step(dev_rows[t % R])
    assert sess.all_done()
    toks = sess.tokens()
    f = sess.fields()
    acc = sess.stats_acc.cpu().numpy()
    for b in range(B):
        assert toks[b] == ref[b][0], (b, toks[b], ref[b][0])
        assert int(f["bit_pos"][b]) == ref[b][1] and int(f["ntokens"][b]) == len(ref[b][0])
        np.testing.assert_allclose(acc[b], ref[b][2], rtol=1e-9, atol=1e-12)  # float64 on both sides
    # decode, lockstep and table-driven
    if mode == "huffman":
        ref_bits = [bc.huffman_decode_stream(lambda t, b=b: rows[t % R, b], toks[b], banned=banned, block_size=block)
                    for b in range(B)]
    else:
        ref_bits = [bc.bins_decode_stream(lambda t, b=b: rows[t % R, b], toks[b], banned=banned, block_size=block,
                                          table=table) for b in range(B)]
    T = max(len(t) for t in toks)
    dec = BaselineDecodeSession(ctx, toks, mode=mode, block_size=block)
    tab = BaselineDecodeStreamsSession(ctx, B, max_tokens=T, mode=mode, block_size=block)
    tab.load_slots(list(range(B)), toks)
    for t in range(T):
        dec.step(dev_rows[t % R])
        tab.step(dev_rows[t % R])
    tab.step(dev_rows[0])  # every slot is past its end: parked, nothing written
    got, counts, flags, nt = tab.harvest(list(range(B)))
    assert dec.bits() == ref_bits
    assert got == ref_bits and not flags.any() and nt.tolist() == [len(t) for t in toks]
    for b in range(B):
        assert bits[b] == ref_bits[b][: len(bits[b])]
        assert len(counts[b]) == len(toks[b]) and all(np.diff([0] + counts[b]) >= 1)  # a token emits >= 1 bit
        assert (counts[b][-1] if counts[b] else 0) == len(ref_bits[b])
    assert tab.out_token.cpu().tolist() == [t[-1] if t else 0 for t in toks]
    ctx.close()


@pytest.mark.parametrize("mode", ["huffman", "bins"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_rows_that_cannot_be_coded_leave_the_state_alone(mode, dtype):
    """NaN, +inf (anywhere but at a banned id) and -inf among the leaders / at a bin's head: NS_ST_ERR_RANGE | DONE,
    state, bits and export untouched; a NaN at a banned id is never read."""
    import torch

    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import BaselineDecodeSession, BaselineEncodeSession

    V, ld, block = 700, 704, 3
    banned = [V - 1, 628]
    base = np.linspace(3.0, -3.0, V).astype(np.float32)
    rows = np.stack([base] * 5)
    rows[0, 400] = np.nan
    rows[1, 7] = np.inf
    rows[2, 5:] = -np.inf      # Huffman: -inf among the 8 leaders; bins: bins led by -inf
    rows[3, 628] = np.nan      # banned: fine
    ctx = _ctx(V, dtype, 5)
    bits = [[1, 0, 1, 1, 0, 1]] * 5
    sess = BaselineEncodeSession(ctx, bits, mode=mode, block_size=block, stats=True)
    tr = sess.enable_trace()
    sess.step(_dev(rows, ld, dtype))
    f = sess.fields()
    bad = _lib.NS_ST_ERR_RANGE | _lib.NS_ST_DONE
    assert f["flags"][:3].tolist() == [bad] * 3 and not (f["flags"][3:] & _lib.NS_ST_ERR_RANGE).any()
    assert f["bit_pos"][:3].tolist() == [0, 0, 0] and f["ntokens"][:3].tolist() == [0, 0, 0]
    assert f["ntokens"][3:].tolist() == [1, 1] and (f["bit_pos"][3:] > 0).all()
    assert (sess.stats_acc[:3].cpu().numpy() == 0).all() and (sess.hist[:3].cpu().numpy() == -1).all()
    assert sess.trace_rows().sel[:3].tolist() == [-1, -1, -1]
    with pytest.raises(Exception):
        sess.tokens()
    table = bc.word2bin_table(V, block)
    good = bc.huffman_encode_stream(lambda t: rows[4], bits[4][:1], banned=banned, block_size=block)[0] \
        if mode == "huffman" else [int(bc.BinsRow(rows[4], banned, block, table).tokens[5])]
    dec = BaselineDecodeSession(ctx, [good[:1]] * 5, mode=mode, block_size=block)
    ranked = dec.enable_export()
    ranked.fill_(-7)
    dec.out_bits.fill_(0xA5)
    dec.step(_dev(rows, ld, dtype))
    from neuralsteganography_amd.coder import _state_fields

    f = _state_fields(dec.state)
    assert f["flags"][:3].tolist() == [bad] * 3 and f["flags"][3:].tolist() == [0, 0]
    assert f["bit_pos"][:3].tolist() == [0, 0, 0] and f["ntokens"][:3].tolist() == [0, 0, 0]
    assert (dec.out_bits[:3].cpu().numpy() == 0xA5).all() and (ranked.cpu().numpy() == -7).all()
    _ = torch
    ctx.close()


@pytest.mark.parametrize("mode,block", [("huffman", 3), ("huffman", 8), ("bins", 3), ("bins", 8)])
def test_divergence_contract_and_export_layouts(mode, block):
    """A token the coder cannot have emitted: state and bits untouched, NS_ST_ERR_DIVERGE | NS_ST_DONE, the K ranked
    leaders (Huffman) / every bin's token in bin order (bins) exported with the terminator rule of
    ``ns_set_rank_export``; the re-issued step under an active mask touches no other stream."""
    from neuralsteganography_amd import _lib
    from neuralsteganography_amd.coder import BaselineStreamingDecodeSession, _state_fields

    V, ld, B, dtype = 700, 704, 5, "f32"
    K = 1 << block
    banned = [V - 1, 628]
    rows = _rows(V, dtype, B, block, 2)
    table = bc.word2bin_table(V, block) if mode == "bins" else None

    def step_ref(row, tok):
        if mode == "huffman":
            return bc.huffman_decode_step(row, tok, banned=banned, block_size=block)
        return bc.bins_decode_step(row, tok, banned=banned, block_size=block, table=table)

    ids = []
    for b in range(B):
        with pytest.raises(bc.Divergence) as e:
            step_ref(rows[0, b], V - 1)  # a banned id is never emitted
        ids.append(e.value.ids)
    # received: stream 0 a good token, 1 a banned id, 2 an id past the vocabulary, 3 a negative id, 4 a low-ranked id
    low = int(bc.ranking(rows[0, 4] + np.float32(0), bc._banned_mask(V, banned))[-3])
    if mode == "bins":  # an id that is not its bin's token
        assert low not in ids[4]
    tokens = [ids[0][1], V - 1, V + 5, -2, low]
    ctx = _ctx(V, dtype, B)
    sess = BaselineStreamingDecodeSession(ctx, B, 4, mode=mode, block_size=block)
    sess.ranked.fill_(-7)
    sess.out_bits.fill_(0x5A)
    lg = _dev(rows[0], ld, dtype)
    sess.step(lg, tokens, [True] * B)
    f = _state_fields(sess.state)
    div = _lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE
    assert f["flags"].tolist() == [0] + [div] * 4
    assert f["bit_pos"][1:].tolist() == [0] * 4 and f["ntokens"].tolist() == [1, 0, 0, 0, 0]
    ob = sess.out_bits.cpu().numpy()
    assert (ob[1:] == 0x5A).all()
    ranked = sess.ranked.cpu().numpy()
    assert (ranked[0] == -7).all(), "a successful step exports nothing"
    for b in range(1, B):
        assert ranked[b, :K].tolist() == ids[b] and ranked[b, K] == -1
        assert sess.ranked_ids(b) == ids[b]
    first = step_ref(rows[0, 0], tokens[0])
    assert sess.bits()[0] == first
    # re-issue streams 1..4 with a token of their export; stream 0 (inactive) must not move
    before = sess.state[0].clone()
    sess.clear([1, 2, 3, 4])
    redo = [0] + [ids[b][(3 * b) % K] for b in range(1, B)]
    sess.step(lg, redo, [False, True, True, True, True])
    assert (sess.state[0] == before).all()
    got = sess.bits()
    for b in range(1, B):
        assert got[b] == step_ref(rows[0, b], redo[b])
    assert sess.diverged() == []
    # a stride of exactly K: K ids and no terminator; nothing of another row
    import torch

    small = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    sess.ranked, sess.rank_stride = small, K
    sess.step(_dev(rows[1], ld, dtype), [V - 1] * B, [False, False, True, False, False])
    out = small.cpu().numpy()
    with pytest.raises(bc.Divergence) as e:
        step_ref(rows[1, 2], V - 1)
    assert out[2].tolist() == e.value.ids and (np.delete(out, 2, axis=0) == -7).all()
    ctx.close()


@pytest.mark.parametrize("name", bc.GOLDEN_STEPS + bc.GOLDEN_FINISH)
def test_goldens_through_the_kernels(name):
    """Every stream the reference coded: its tokens, statistics and decoded bits from the kernels."""
    from neuralsteganography_amd.coder import baseline_decode_batch, baseline_encode_batch, row_stride

    g = bc.Golden(name)
    dtype = g.meta["dtype"]
    ld = row_stride(g.vocab, dtype)
    ctx = _ctx(g.vocab, dtype, 1)
    if g.sent_end is not None:
        ctx.set_sentence_end(g.sent_end.astype(np.uint8))
    for s in range(g.n):
        fn = lambda t, _last=None, s=s: _dev(g.row(s, t)[None, :], ld, dtype)  # noqa: E731
        toks, st = baseline_encode_batch(ctx, [g.msg[s]], fn, mode=g.coder, block_size=g.blocks[s],
                                         finish_sent=g.sent_end is not None, return_stats=True, check_every=1)
        assert toks[0] == g.tokens[s], (name, s)
        got = (st[0]["avg_NLL"], st[0]["avg_KL"], st[0]["words_per_bit"])
        print(name, s, got, g.stats[s].tolist())
        np.testing.assert_allclose(got, g.stats[s], rtol=STAT_RTOL)
        bits = baseline_decode_batch(ctx, [g.tokens[s]], fn, mode=g.coder, block_size=g.blocks[s])
        assert bits[0] == g.bits[s], (name, s)
    ctx.close()


def test_block_size_errors_on_the_device_path():
    from neuralsteganography_amd.coder import BaselineEncodeSession, CoderContext, CoderParams
    from neuralsteganography_amd.exceptions import ConfigurationError

    ctx = CoderContext(CoderParams(vocab=258, banned=[257, 3, 4], topk=2), max_batch=2, device=0)
    for block in (0, 9, 8):  # 8: 256 leaders, 255 ids left
        with pytest.raises(ConfigurationError):
            BaselineEncodeSession(ctx, [[1, 0]], mode="huffman", block_size=block)
    with pytest.raises(ConfigurationError):
        BaselineEncodeSession(ctx, [[1, 0]], mode="rank", block_size=3)
    ctx.close()


# ---------------------------------------------------------------------------------------------- tiny native GPT-2
def _tiny():
    from neuralsteganography_amd.lm.gpt2 import random_gpt2

    return random_gpt2("tiny", n_layer=2, n_head=2, n_embd=128, vocab_size=512, n_positions=256)


def _provider():
    import torch

    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    return HipArithmeticLM(_tiny(), None, logits_dtype="f16", compute_dtype=torch.float16)


def _messages(n=12):
    """12 payloads of 150-200 bits; 12 contexts: 2 and 5 equal, 8 and 9 equal, 0 and 7 share a 64-token prefix."""
    rng = np.random.default_rng(77)
    bits = [rng.integers(0, 2, size=int(k)).tolist() for k in rng.integers(150, 201, size=n)]
    base = rng.integers(0, 511, size=64).tolist()
    ctxs = [rng.integers(0, 511, size=int(k)).tolist() for k in rng.integers(3, 45, size=n)]
    ctxs[0] = base + ctxs[0][:3]
    ctxs[7] = base + ctxs[7][:6]
    ctxs[5] = list(ctxs[2])
    ctxs[9] = list(ctxs[8])
    return bits, ctxs


@pytest.mark.parametrize("mode,block", [("huffman", 3), ("bins", 2)])
def test_slot_batch_equals_each_message_alone(mode, block):
    """12 messages, 12 contexts, 4 slots and a page budget that forces an eviction: tokens and statistics equal each
    message's own one-message call; decode recovers every payload."""
    bits, ctxs = _messages()
    alone = _provider()
    ref, ref_st = [], []
    for b, c in zip(bits, ctxs):
        t, s = alone.encode_baseline_batch([b], c, mode=mode, block_size=block, return_stats=True)
        ref.append(t[0])
        ref_st.append(s[0])
    assert all(40 <= len(t) <= 180 for t in ref), [len(t) for t in ref]
    lm = _provider()
    lm.lm.kv_segment_pages = 1  # a page-exact budget
    pool = lm.lm.page_pool()
    # pages hold 32 positions.  A message is 40-180 tokens after a context of up to 70 (at most 250 positions: eight
    # pages, so any one fits); four are admitted on one to three pages each (context + 17 positions) and every one
    # grows by at least 40 positions -- at least one more page each -- which eight pages cannot hold at once
    cap_pages = 8
    pool.budget_bytes = lambda: (cap_pages - pool.total) * pool.page_bytes
    got, st = lm.encode_baseline_batch(bits, contexts=ctxs, mode=mode, block_size=block, return_stats=True, slots=4)
    sched = lm.last_schedule
    assert got == ref
    assert sched["slots"] == 4 and sched["evictions"] > 0 and sched["kv_pages_peak"] <= cap_pages, sched
    for a, b in zip(st, ref_st):
        assert a == b, (a, b)  # the same float64 accumulations in the same order
    assert pool.free_pages == pool.total
    out = lm.decode_baseline_batch(got, contexts=ctxs, mode=mode, block_size=block, slots=4)
    assert [o[: len(b)] for o, b in zip(out, bits)] == bits
    assert all(len(o) - len(b) < (1 << block) for o, b in zip(out, bits))
    assert pool.free_pages == pool.total
    # eager, unlimited pages: the same again (graph capture changes nothing)
    free = _provider()
    assert free.encode_baseline_batch(bits, contexts=ctxs, mode=mode, block_size=block, slots=4, graphs=False) == ref
    assert free.last_schedule["evictions"] == 0
    out2, _ = free.decode_baseline_repair(got, contexts=ctxs, mode=mode, block_size=block)
    assert out2 == out


# ---------------------------------------------------------------------------------------------- code_base entries
@pytest.mark.parametrize("coder", ["huffman", "bins"])
def test_code_base_entry_points_return_the_reference_tuples(coder):
    """``encode_huffman`` / ``encode_block`` over the golden's synthetic rows: the reference's (tokens, avg_NLL,
    avg_KL, words_per_bit); ``decode_*`` of the reference's tokens: its bits."""
    from neuralsteganography_amd import code_base, synthetic

    g = bc.Golden("bh_v700_f32" if coder == "huffman" else "bb_v700_f32")
    ctx_ids = synthetic.DEFAULT_CONTEXT
    for s in range(g.n):
        lm = synthetic.SyntheticBatchedLM(g.meta["logit_seed"], g.vocab, g.meta["scale"], "f32", streams=[s])
        enc = bc.PresetEnc(None, g.tokens[s])
        if coder == "huffman":
            res = code_base.encode_huffman(lm, enc, g.msg[s], ctx_ids, g.blocks[s])
            bits = code_base.decode_huffman(lm, enc, "", ctx_ids, g.blocks[s])
        else:
            b2w, w2b = code_base.get_bins(g.vocab, g.blocks[s])
            res = code_base.encode_block(lm, enc, g.msg[s], ctx_ids, g.blocks[s], b2w, w2b)
            bits = code_base.decode_block(lm, enc, "", ctx_ids, g.blocks[s], b2w, w2b)
        assert len(res) == 4 and res[0] == g.tokens[s]
        np.testing.assert_allclose(res[1:], g.stats[s], rtol=STAT_RTOL)
        assert bits == g.bits[s]


@pytest.mark.parametrize("coder", ["huffman", "bins"])
def test_code_base_text_decode_reproduces_the_repair_goldens(coder):
    from neuralsteganography_amd import code_base, synthetic
    from tests.golden.toy_tokenizer import ToyTokenizer

    g = bc.Golden("bh_text_v700" if coder == "huffman" else "bb_text_v700")
    toy = ToyTokenizer(g.vocab)
    for s in range(g.n):
        spec = g.meta["streams"][s]
        boost = {spec["at"]: spec["boost"]} if "boost" in spec else None
        lm = synthetic.SyntheticBatchedLM(g.meta["logit_seed"], g.vocab, g.meta["scale"], "f32", streams=[s],
                                          boost=boost)
        enc = bc.PresetEnc(toy, g.tokens[s])
        if coder == "huffman":
            bits = code_base.decode_huffman(lm, enc, "", synthetic.DEFAULT_CONTEXT, g.blocks[s])
        else:
            bits = code_base.decode_block(lm, enc, "", synthetic.DEFAULT_CONTEXT, g.blocks[s])
        assert bits == g.bits[s], (coder, s)
