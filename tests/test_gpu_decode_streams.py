"""GPU: the decode step with per-stream token rows (``ns_decode_step_streams``, ``coder.DecodeStreamsSession``), the
kernel entry alone on synthetic logit rows.

The contract: a stream's states, bits and bit counts are those ``ns_decode_step`` gives it with the same quality table
registered, step by step, and those of the CPU oracle run with the stream's own (temp, topk, precision); the stream's
token index is its own ``ntokens``, so nothing depends on the row it runs in; a stream past its length, or flagged
done, is parked -- nothing of it is written.  Every comparison is exact.

Token streams come from the oracle's encoder (a random payload under the stream's own quality), so every token is
inside the kept top-k until one is planted outside it.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neuralsteganography_amd import _lib, synthetic  # noqa: E402
from neuralsteganography_amd.coder import (CoderContext, CoderParams, DecodeSession, DecodeStreamsSession,  # noqa: E402
                                           StreamQuality, _state_fields, row_stride)
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, SCALE, NMAX, T = 77, 3.0, 37, 6
# ragged lengths: stream 1 is parked from the start, stream 2's first token is its last (the flush on the first
# step), stream 3 ends in the middle of the run, stream 4 runs to the end
LENS = [5, 0, 1, 3, 6] + [(3 * s) % 7 for s in range(5, NMAX)]
assert max(LENS) == T and len(LENS) == NMAX
# three distinct (temp, topk, precision), assigned round robin
Q_SINGLE = [(0.9, 300, 26), (0.7, 40, 16), (1.3, 2, 40)]
Q_WIDE = [(1.0, 50000, 26), (0.8, 600, 16), (1.2, 40, 40)]  # k_max 50,000: the wide chain serves every row


def _banned(V):
    return [V - 1, 628]


def _npdt(dtype):
    return np.float16 if dtype == "f16" else np.float32


def _limit(dtype):
    return _lib.max_topk(_lib.NS_DTYPE_F16 if dtype == "f16" else _lib.NS_DTYPE_F32)


def _row(V, dtype, s, t):
    return synthetic.logits_row(SEED, s, t, V, SCALE, _npdt(dtype)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(V, dtype, wide):
    """Per (vocabulary, dtype, path), computed once on the CPU for all 37 streams: the token lists (oracle encode of
    a random payload), and the oracle's decode of them -- bit_pos after every token and the emitted bits."""
    qs = [(Q_WIDE if wide else Q_SINGLE)[s % 3] for s in range(NMAX)]
    toks, counts, bits = [], [], []
    for s in range(NMAX):
        temp, topk, prec = qs[s]
        kw = dict(banned=_banned(V), temp=temp, precision=prec, topk=topk)
        pl = synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(500 + s, 64))
        packed = np.packbits(np.asarray(pl, dtype=np.uint8), bitorder="little")
        st, tl = oracle.new_state(prec), []
        for t in range(LENS[s]):
            rc, tok, _ = oracle.encode_step(_row(V, dtype, s, t), st, packed, len(pl), **kw)
            assert rc == 0 and st.bit_pos < len(pl)
            tl.append(int(tok))
        st, cn = oracle.new_state(prec), []
        out = np.zeros((T * 60 + 7) // 8 + 8, dtype=np.uint8)
        for t, tok in enumerate(tl):
            rc, _ = oracle.decode_step(_row(V, dtype, s, t), st, tok, t == len(tl) - 1, out, **kw)
            assert rc == 0
            cn.append(int(st.bit_pos))
        toks.append(tl)
        counts.append(cn)
        bits.append(np.unpackbits(out, bitorder="little")[: st.bit_pos].tolist())
    return qs, toks, counts, bits


@functools.lru_cache(maxsize=None)
def _device_rows(V, dtype, B):
    """[T, B, ld] logits on the device: row (t, s) is stream s's row at ITS token index t."""
    ld = row_stride(V, dtype)
    return torch.from_numpy(np.stack([synthetic.logits_batch(SEED, range(B), t, V, SCALE, _npdt(dtype), ld)
                                      for t in range(T)])).cuda()


def _quality(V, dtype, qs):
    return StreamQuality([CoderParams(vocab=V, precision=p, temp=t, topk=k, dtype=dtype) for t, k, p in qs])


def _rows_at(rows, tidx):
    """The step's [B, ld] matrix: stream b's row at token index tidx[b] (clamped: a parked stream's row is unused)."""
    B = rows.shape[1]
    ti = torch.as_tensor(np.clip(np.asarray(tidx, dtype=np.int64), 0, T - 1), device=rows.device)
    return rows[ti, torch.arange(B, device=rows.device)].contiguous()


def _session(ctx, sq, toks, slots=None):
    B = len(toks)
    sess = DecodeStreamsSession(ctx, B, max_tokens=T, k_max=sq.k_max, max_precision=sq.max_precision)
    sess.load_slots(np.arange(B) if slots is None else slots, toks, sq)
    return sess


def _buffers(sess):
    torch.cuda.synchronize()
    return {k: getattr(sess, k).cpu().numpy().copy()
            for k in ("state", "out_bits", "counts", "out_token", "ranked", "trace") if getattr(sess, k) is not None}


def _bits_of(buf, b):
    bp = int(buf["state"][b, 2])
    return np.unpackbits(buf["out_bits"][b], bitorder="little")[:bp].tolist()


def _check_against_scalar_and_oracle(V, dtype, wide, B):
    qs, toks, counts, bits = _reference(V, dtype, wide)
    qs, toks, counts, bits = qs[:B], toks[:B], counts[:B], bits[:B]
    lens = np.asarray(LENS[:B])
    rows = _device_rows(V, dtype, NMAX)[:, :B]
    sq = _quality(V, dtype, qs)
    assert (min(sq.k_max, V - 1) > _limit(dtype)) == wide
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _session(ctx, sq, toks)
    sess.enable_trace()
    parked = [b for b in range(B) if lens[b] == 0]
    if parked:  # a stream parked from the start sits on sentinel values throughout
        pi = torch.as_tensor(parked, device="cuda")
        sess.state[pi] = torch.tensor([0x1111, 0x2222, 3, 0], dtype=torch.int64, device="cuda")
        sess.out_bits[pi] = 0xA5
        sess.counts[pi] = -7
        sess.out_token[pi] = -9
        sess.trace[pi] = -11
    sentinel = _buffers(sess)
    scalar = DecodeSession(ctx, toks, quality=sq)
    live = [b for b in range(B) if b not in parked]
    for t in range(T):
        logits = rows[t].contiguous()  # every stream starts at step 0: its token index is the step while it runs
        out = sess.step(logits)
        if t < scalar.T:
            scalar.step(logits)
        got = _buffers(sess)
        ref = scalar.state.cpu().numpy()
        assert np.array_equal(got["state"][live], ref[live]), f"step {t}: states differ from ns_decode_step"
        assert out.data_ptr() == sess.out_token.data_ptr()
        for b in live:
            n = min(t + 1, int(lens[b]))
            assert got["counts"][b, :n].tolist() == counts[b][:n], (t, b)
            assert not got["counts"][b, n:].any(), (t, b)  # nothing past the tokens decoded so far
            if n:
                assert int(got["out_token"][b]) == toks[b][n - 1], (t, b)
                assert int(got["state"][b, 2]) == counts[b][n - 1]
    ref_bits = scalar.out_bits.cpu().numpy()
    for b in live:
        assert _state_fields(torch.from_numpy(got["state"][b:b + 1]))["ntokens"][0] == lens[b]
        assert _bits_of(got, b) == bits[b], f"stream {b}: bits differ from the oracle"
        nb = (counts[b][-1] + 7) // 8
        assert np.array_equal(got["out_bits"][b, :nb], ref_bits[b, :nb]), f"stream {b}: bits differ from ns_decode_step"
    hb, hc, hf, hn = sess.harvest(np.arange(B))
    assert [hb[b] for b in live] == [bits[b] for b in live] and [hc[b] for b in live] == [counts[b] for b in live]
    assert not (hf[live] & ~np.uint32(_lib.NS_ST_EXACT_SUM)).any()
    assert hn[live].tolist() == lens[live].tolist()
    for _ in range(8):  # every stream is past its end now: further steps write nothing at all
        sess.step(rows[T - 1].contiguous())
    after = _buffers(sess)
    for k, v in got.items():
        assert np.array_equal(after[k], v), f"{k} changed on a parked stream"
    for k, v in sentinel.items():
        assert np.array_equal(after[k][parked], v[parked]), f"{k} of the stream parked from the start changed"


@pytest.fixture(params=["wave", "auto"])
def form(request):
    """The wave-per-stream form, and the automatic choice (with the speculative sample on -- V = 50,257 -- the split
    form: one workgroup per stream)."""
    prev = _lib.set_split_max_batch(0 if request.param == "wave" else -1)
    yield request.param
    _lib.set_split_max_batch(prev)


@pytest.mark.parametrize("B", [1, 5, 37])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("V", [65, 640, 50257])
def test_single_pass_equals_scalar_entry_and_oracle(V, dtype, B, form):
    _check_against_scalar_and_oracle(V, dtype, False, B)


@pytest.mark.parametrize("B", [1, 5, 37])
@pytest.mark.parametrize("V,dtype", [(515, "f16"), (771, "f32"), (50257, "f32"), (50257, "f16")])
def test_wide_chain_equals_scalar_entry_and_oracle(V, dtype, B):
    _check_against_scalar_and_oracle(V, dtype, True, B)


@pytest.mark.parametrize("V,dtype,wide", [(640, "f32", False), (50257, "f16", False), (771, "f32", True)])
def test_permuting_the_rows_permutes_the_outputs(V, dtype, wide):
    B = 5
    qs, toks, counts, bits = (x[:B] for x in _reference(V, dtype, wide))
    perm = [3, 0, 4, 2, 1]  # row r runs stream perm[r]
    rows = _device_rows(V, dtype, NMAX)[:, perm]
    sq = _quality(V, dtype, qs)
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _session(ctx, sq.take(perm), [toks[s] for s in perm])
    for t in range(T):
        sess.step(rows[t].contiguous())
    hb, hc, hf, hn = sess.harvest(np.arange(B))
    assert hb == [bits[s] for s in perm] and hc == [counts[s] for s in perm]
    assert hn.tolist() == [LENS[s] for s in perm]


@pytest.mark.parametrize("V,dtype,wide", [(640, "f32", False), (50257, "f16", False), (771, "f32", True)])
def test_planted_token_outside_the_top_k_diverges_and_continues(V, dtype, wide):
    B, bad, at = 5, 4, 2  # stream 4 (6 tokens) receives, as its token 2, the id of its row's smallest logit
    qs, toks, counts, bits = (x[:B] for x in _reference(V, dtype, wide))
    temp, topk, prec = qs[bad]
    row = _row(V, dtype, bad, at)
    row[_banned(V)[0]] = np.inf
    planted = int(np.argmin(row))
    st = oracle.new_state(prec)
    scratch = np.zeros(64, dtype=np.uint8)
    for t in range(at):
        oracle.decode_step(_row(V, dtype, bad, t), st, toks[bad][t], False, scratch, banned=_banned(V), temp=temp,
                           precision=prec, topk=topk)
    rc, _, kept = oracle.decode_step_kept(_row(V, dtype, bad, at), st, planted, False, scratch, banned=_banned(V),
                                          temp=temp, precision=prec, topk=topk)
    assert rc == oracle.OR_ERR_DIVERGE and planted not in kept and len(kept) >= 2
    rows = _device_rows(V, dtype, NMAX)[:, :B]
    sq = _quality(V, dtype, qs)
    ctx = CoderContext(sq.context_params(), max_batch=B)
    given = [list(tl) for tl in toks]
    given[bad][at] = planted
    sess = _session(ctx, sq, given)
    sess.ranked.fill_(-5)
    tidx = np.zeros(B, dtype=np.int64)
    for t in range(at):
        sess.step(_rows_at(rows, tidx))
        tidx += 1
    before = _buffers(sess)
    for extra in range(2):  # the diverging step, then one more on the parked stream
        sess.step(_rows_at(rows, tidx))
        tidx[np.arange(B) != bad] += 1
        got = _buffers(sess)
        f = _state_fields(torch.from_numpy(got["state"]))
        assert int(f["flags"][bad]) & (_lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE) == \
            _lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE
        assert got["state"][bad, :3].tolist() == before["state"][bad, :3].tolist()  # lo, hi, bit_pos
        assert int(f["ntokens"][bad]) == at
        for k in ("out_bits", "counts", "out_token"):
            assert np.array_equal(got[k][bad], before[k][bad]), f"{k} of the diverged stream changed"
        n = min(len(kept), sess.rank_stride)
        assert got["ranked"][bad, :n].tolist() == kept[:n]
        if len(kept) < sess.rank_stride:
            assert got["ranked"][bad, len(kept)] == -1 and (got["ranked"][bad, len(kept) + 1:] == -5).all()
        others = [b for b in range(B) if b != bad]
        assert (got["ranked"][others] == -5).all()  # no other row is written
        for b in others:  # the other streams went on as if nothing had happened
            n = min(at + 1 + extra, LENS[b])
            assert got["counts"][b, :n].tolist() == counts[b][:n]
    sess.clear([bad], tokens=[toks[bad][at]])
    for _ in range(T):
        sess.step(_rows_at(rows, tidx))
        torch.cuda.synchronize()
        tidx = np.minimum(_state_fields(sess.state)["ntokens"].astype(np.int64), T - 1)
    hb, hc, hf, hn = sess.harvest(np.arange(B))
    live = [b for b in range(B) if LENS[b]]
    assert [hb[b] for b in live] == [bits[b] for b in live] and [hc[b] for b in live] == [counts[b] for b in live]
    assert not (hf & (_lib.NS_ST_ERR_DIVERGE | _lib.NS_ST_DONE)).any()


def test_refused_arguments():
    V, dtype, B = 640, "f32", 5
    qs, toks, _, _ = (x[:B] for x in _reference(V, dtype, False))
    rows = _device_rows(V, dtype, NMAX)[:, :B]
    sq = _quality(V, dtype, qs)
    ctx = CoderContext(sq.context_params(), max_batch=B)
    sess = _session(ctx, sq, toks)
    L = _lib.lib()
    logits = rows[0].contiguous()

    def call(h=ctx, **kw):
        a = dict(quality=sess.qtable.data_ptr(), k_max=sess.k_max, tokens=sess.tokmat.data_ptr(), tok_stride=T,
                 length=sess.nlen.data_ptr(), counts=sess.counts.data_ptr(), counts_stride=T,
                 out_token=sess.out_token.data_ptr())
        a.update(kw)
        return L.ns_decode_step_streams(h._h if h is not None else None, logits.data_ptr(), logits.stride(0), B,
                                        a["quality"], a["k_max"], a["tokens"], a["tok_stride"], a["length"],
                                        sess.state.data_ptr(), sess.out_bits.data_ptr(), sess.out_stride, a["counts"],
                                        a["counts_stride"], a["out_token"], ctx._banned, ctx._nbanned, None, 0, None)

    assert call(h=None) == _lib.NS_ERR_CONFIG
    for name in ("quality", "tokens", "length", "counts", "out_token"):
        assert call(**{name: None}) == _lib.NS_ERR_CONFIG, name
    assert call(quality=sess.qtable.data_ptr() + 4) == _lib.NS_ERR_CONFIG
    assert call(counts=sess.counts.data_ptr() + 4) == _lib.NS_ERR_CONFIG
    for name in ("tokens", "length", "out_token"):
        assert call(**{name: getattr(sess, {"tokens": "tokmat", "length": "nlen"}.get(name, name)).data_ptr() + 2}) \
            == _lib.NS_ERR_CONFIG, name
    for kw in (dict(k_max=0), dict(tok_stride=0), dict(counts_stride=0)):
        assert call(**kw) == _lib.NS_ERR_CONFIG, kw
    f64 = CoderContext(CoderParams(vocab=V, precision=26, topk=300, dtype="f64"), max_batch=B)
    assert call(h=f64) == _lib.NS_ERR_CONFIG
    assert L.ns_set_stream_quality(ctx._h, sess.qtable.data_ptr(), sess.k_max) == _lib.NS_OK
    try:
        assert call() == _lib.NS_ERR_CONFIG  # a registered table, as ns_sample_step_streams
    finally:
        assert L.ns_set_stream_quality(ctx._h, None, 0) == _lib.NS_OK
    before = _buffers(sess)
    assert call() == _lib.NS_OK
    assert not np.array_equal(_buffers(sess)["state"], before["state"])  # the accepted call does run the step
