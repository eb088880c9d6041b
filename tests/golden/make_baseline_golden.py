"""Generate the baseline-coder golden vectors by running the REFERENCE's ``code_base/huffman_baseline.py`` (with
``huffman.py``) and ``code_base/block_baseline.py``, with the shims of ``make_golden.py``: a synthetic model that
returns ``(logits, past)``, ``torch.sort`` forced stable (value desc, id asc), a stub tokenizer and
``device="cpu"``.  Rows are fp32 tensors; the "f16" cases hold fp16-valued rows (ties are common).

For every stream the script asserts that the restatement (``tests/baseline_cases.py``) reproduces the reference's
tokens and decoded bits exactly BEFORE writing the fixture; if it does not, the script fails (pick another seed:
the canonical fp32 weights differ from torch's in the last ulp, DESIGN.md "Deviations").  The text-decode cases
feed a preset received-token list (a cover text re-tokenised by the toy tokenizer, or one with a token replaced) so
that every branch of the two files' BPE repairs runs; the branches hit are asserted and recorded.

Usage: ``python tests/golden/make_baseline_golden.py`` (well under a minute).
"""

from __future__ import annotations

import contextlib
import io
import json
import sys
import types
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))

from neuralsteganography_amd import synthetic  # noqa: E402
from tests import baseline_cases as bc  # noqa: E402

LOGIT_SEED = 11
BLOCK_NBITS = {1: 23, 3: 40, 5: 33, 8: 52}  # ends mid-code (Huffman) and mid-block (bins: 40 % 3, 33 % 5, 52 % 8)

# name: vocab, row dtype, logit scale; one stream per block size
STEP_CONFIGS = {
    "v700_f32": dict(vocab=700, dtype="f32", scale=2.0),
    "v700_f16": dict(vocab=700, dtype="f16", scale=2.0),
    "v50257_f32": dict(vocab=50257, dtype="f32", scale=3.0),
    "v50257_f16": dict(vocab=50257, dtype="f16", scale=3.0),
}
FINISH_CONFIG = dict(vocab=50257, dtype="f32", scale=3.0, block=3, nbits=[17, 9])
# text decode over the toy tokenizer: stream -> (block, nbits, edit); an edit replaces the received token at `at`
# with `token` and boosts id `boost` (+30) at that step
TEXT_STREAMS = [
    dict(block=3, nbits=60), dict(block=5, nbits=70), dict(block=3, nbits=48), dict(block=2, nbits=40),
    dict(block=3, nbits=30, at=4, token=128, boost=198),   # huffman_baseline.py:113 (128 -> 198)
    dict(block=3, nbits=30, at=5, token=26),               # " ": no leader is a prefix of it or starts with it
]
TEXT_VOCAB, TEXT_SCALE = 700, 2.0


def row_of(cfg, stream, t, boost=None):
    dtype = np.float16 if cfg["dtype"] == "f16" else np.float32
    row = synthetic.logits_row(LOGIT_SEED, stream, t, cfg["vocab"], cfg["scale"], dtype).astype(np.float32)
    if boost and t in boost:
        row = row.copy()
        row[boost[t]] += np.float32(30.0)
    return row


class Model:
    """``logits, past = model(prev.unsqueeze(0), past=past)``: call t returns row t of the stream."""

    def __init__(self, cfg, stream, boost=None):
        self.cfg, self.stream, self.boost, self.calls = cfg, stream, boost, 0

    def __call__(self, input_ids, past=None):
        import torch

        row = row_of(self.cfg, self.stream, self.calls, self.boost)
        self.calls += 1
        logits = torch.zeros((1, int(input_ids.shape[-1]), self.cfg["vocab"]), dtype=torch.float32)
        logits[0, -1] = torch.from_numpy(row.copy())
        return logits, ()


class StubTokenizer:
    """decode(): "." for sentence-ending ids (id % 97 == 5), else "a"; encode(): the preset token list."""

    def __init__(self, tokens=None):
        self.tokens = list(tokens or [])

    def decode(self, ids):
        return "".join("." if int(i) % 97 == 5 else "a" for i in ids)

    def encode(self, text):
        return list(self.tokens)


def _import_reference():
    import torch
    from torch.overrides import TorchFunctionMode

    sys.modules.setdefault("bitarray", types.ModuleType("bitarray"))
    sys.path.insert(0, str(REF / "code_base"))
    import block_baseline as ref_b
    import huffman_baseline as ref_h

    assert Path(ref_h.__file__).resolve() == (REF / "code_base" / "huffman_baseline.py").resolve()
    assert Path(ref_b.__file__).resolve() == (REF / "code_base" / "block_baseline.py").resolve()

    class StableSort(TorchFunctionMode):
        def __torch_function__(self, func, types_, args=(), kwargs=None):
            kwargs = dict(kwargs or {})
            if func in (torch.Tensor.sort, torch.sort):
                kwargs["stable"] = True
            return func(*args, **kwargs)

    return ref_h, ref_b, StableSort


def message(stream, nbits):
    return synthetic.bytes_to_bits_lsb(synthetic.payload_bytes(stream, (nbits + 7) // 8))[:nbits]


def run_stream(coder, ref_h, ref_b, stable, cfg, stream, block, nbits, finish=False):
    """One stream through the reference and through the restatement; returns the fixture row."""
    V = cfg["vocab"]
    banned = [V - 1, 628]
    msg = message(stream, nbits)
    context = synthetic.DEFAULT_CONTEXT
    enc = StubTokenizer()
    model = Model(cfg, stream)
    with stable():
        if coder == "huffman":
            toks, nll, kl, wpb = ref_h.encode_huffman(model, enc, list(msg), context, block, finish_sent=finish,
                                                     device="cpu")
        else:
            b2w, w2b = ref_b.get_bins(V, block)
            toks, nll, kl, wpb = ref_b.encode_block(model, enc, list(msg), context, block, b2w, w2b,
                                                   finish_sent=finish, device="cpu")
        dmodel = Model(cfg, stream)
        if coder == "huffman":
            bits = ref_h.decode_huffman(dmodel, StubTokenizer(toks), "", context, block, device="cpu")
        else:
            bits = ref_b.decode_block(dmodel, StubTokenizer(toks), "", context, block, b2w, w2b, device="cpu")
    sent_end = np.asarray([i % 97 == 5 for i in range(V)]) if finish else None

    def row_fn(t):
        return row_of(cfg, stream, t)

    if coder == "huffman":
        r_toks, r_i, acc = bc.huffman_encode_stream(row_fn, msg, banned=banned, block_size=block, sent_end=sent_end)
        r_bits = bc.huffman_decode_stream(row_fn, toks, banned=banned, block_size=block)
    else:
        table = bc.word2bin_table(V, block)
        assert all(int(table[w]) == b for w, b in w2b.items()), "get_bins restatement differs from the reference"
        r_toks, r_i, acc = bc.bins_encode_stream(row_fn, msg, banned=banned, block_size=block, table=table,
                                                 sent_end=sent_end)
        r_bits = bc.bins_decode_stream(row_fn, toks, banned=banned, block_size=block, table=table)
    assert r_toks == list(toks), f"{coder} stream {stream} block {block}: restated tokens differ from the reference"
    assert r_bits == list(bits), f"{coder} stream {stream} block {block}: restated bits differ from the reference"
    assert list(bits)[:nbits] == list(msg), "reference round trip failed"
    print(f"  {coder} V={V} {cfg['dtype']} block={block} nbits={nbits} tokens={len(toks)} bits={len(bits)} "
          f"i={r_i} NLL={nll:.4f} KL={kl:.4f}", flush=True)
    return dict(tokens=list(toks), bits=list(bits), msg=list(msg), stats=[nll, kl, wpb], block=block, consumed=r_i)


def pack(rows):
    out = {k: [] for k in ("tokens", "bits", "msg")}
    off = {k: [0] for k in out}
    for r in rows:
        for k in out:
            out[k] += r[k]
            off[k].append(len(out[k]))
    arrays = dict(tokens=np.asarray(out["tokens"], np.int32), tok_off=np.asarray(off["tokens"], np.int64),
                  bits=np.asarray(out["bits"], np.uint8), bit_off=np.asarray(off["bits"], np.int64),
                  msg=np.asarray(out["msg"], np.uint8), msg_off=np.asarray(off["msg"], np.int64),
                  stats=np.asarray([r["stats"] for r in rows], np.float64),
                  blocks=np.asarray([r["block"] for r in rows], np.int32),
                  consumed=np.asarray([r["consumed"] for r in rows], np.int64))
    return arrays


def save(name, meta, arrays):
    np.savez_compressed(HERE / f"{name}.npz", meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)


class ToyEnc:
    """The toy tokenizer behind the attributes the two reference files use: ``decoder[id]``, ``encode`` (the first
    call returns the preset received list, later calls tokenise a suffix), ``decode``."""

    def __init__(self, toy, received):
        self.toy, self.received, self.first = toy, list(received), True
        self.decoder = {i: s for i, s in enumerate(toy.pieces)}

    def encode(self, text):
        if self.first:
            self.first = False
            return list(self.received)
        return self.toy.encode(text)

    def decode(self, ids):
        return self.toy.decode(ids)


def run_text(coder, ref_h, ref_b, stable):
    from tests.golden.toy_tokenizer import ToyTokenizer

    toy = ToyTokenizer(TEXT_VOCAB)
    cfg = dict(vocab=TEXT_VOCAB, dtype="f32", scale=TEXT_SCALE)
    banned = [TEXT_VOCAB - 1, 628]
    context = synthetic.DEFAULT_CONTEXT
    rows, tags_seen = [], set()
    for s, spec in enumerate(TEXT_STREAMS):
        block, nbits = spec["block"], spec["nbits"]
        boost = {spec["at"]: spec["boost"]} if "boost" in spec else None
        msg = message(s, nbits)
        with stable():
            if coder == "huffman":
                toks = ref_h.encode_huffman(Model(cfg, s, boost), StubTokenizer(), list(msg), context, block,
                                            device="cpu")[0]
            else:
                b2w, w2b = ref_b.get_bins(TEXT_VOCAB, block)
                toks = ref_b.encode_block(Model(cfg, s, boost), StubTokenizer(), list(msg), context, block, b2w, w2b,
                                          device="cpu")[0]
        received = toy.encode(toy.decode(toks))
        if "at" in spec:
            received = list(toks)
            received[spec["at"]] = spec["token"]
        with stable(), contextlib.redirect_stdout(io.StringIO()):
            if coder == "huffman":
                bits = ref_h.decode_huffman(Model(cfg, s, boost), ToyEnc(toy, received), "", context, block,
                                            device="cpu")
            else:
                bits = ref_b.decode_block(Model(cfg, s, boost), ToyEnc(toy, received), "", context, block, b2w, w2b,
                                          device="cpu")

        def row_fn(t, s=s, boost=boost):
            return row_of(cfg, s, t, boost)

        r_bits, tags, final = bc.decode_text_tokens(coder, row_fn, toy, received, banned=banned, block_size=block)
        assert r_bits == list(bits), f"{coder} text stream {s}: restated bits differ from the reference"
        tags_seen |= set(tags)
        print(f"  {coder} text s={s} block={block} emitted={len(toks)} received={len(received)} "
              f"decoded={len(final)} bits={len(bits)} repairs={tags}", flush=True)
        rows.append(dict(tokens=list(received), bits=list(bits), msg=list(msg), stats=[0.0, 0.0, 0.0], block=block,
                         consumed=len(final), emitted=list(toks), boost=boost))
    need = {"prefix", "longer", "unrepairable"} | ({"n128"} if coder == "huffman" else set())
    assert need <= tags_seen, f"{coder}: repair branches not exercised: {sorted(need - tags_seen)}"
    arrays = pack(rows)
    emitted = [r["emitted"] for r in rows]
    arrays["emitted"] = np.asarray(sum(emitted, []), np.int32)
    arrays["emit_off"] = np.asarray(np.cumsum([0] + [len(e) for e in emitted]), np.int64)
    meta = dict(kind="text", coder=coder, vocab=TEXT_VOCAB, dtype="f32", scale=TEXT_SCALE, logit_seed=LOGIT_SEED,
                streams=TEXT_STREAMS, banned=banned, context=synthetic.DEFAULT_CONTEXT, tokenizer="ToyTokenizer",
                branches=sorted(tags_seen))
    save(f"b{coder[0]}_text_v700", meta, arrays)


def main():
    ref_h, ref_b, stable = _import_reference()
    for coder in ("huffman", "bins"):
        for name, cfg in STEP_CONFIGS.items():
            rows = [run_stream(coder, ref_h, ref_b, stable, cfg, s, block, nbits)
                    for s, (block, nbits) in enumerate(BLOCK_NBITS.items())]
            meta = dict(cfg, kind="steps", coder=coder, logit_seed=LOGIT_SEED, banned=[cfg["vocab"] - 1, 628],
                        payload_seed=synthetic.PAYLOAD_SEED, sort="stable (value desc, id asc)",
                        reference="code_base/huffman_baseline.py" if coder == "huffman"
                        else "code_base/block_baseline.py")
            save(f"b{coder[0]}_{name}", meta, pack(rows))
        cfg = FINISH_CONFIG
        rows = [run_stream(coder, ref_h, ref_b, stable, cfg, s, cfg["block"], nbits, finish=True)
                for s, nbits in enumerate(cfg["nbits"])]
        meta = dict({k: v for k, v in cfg.items() if k != "nbits"}, kind="finish", coder=coder,
                    logit_seed=LOGIT_SEED, banned=[cfg["vocab"] - 1, 628], sent_end="id % 97 == 5")
        save(f"b{coder[0]}_finish_v50257", meta, pack(rows))
        run_text(coder, ref_h, ref_b, stable)
    tables = {}
    for V, block in ((50257, 3), (700, 8)):
        np.random.seed(12345)
        before = np.random.get_state()[1].copy()
        _, w2b = ref_b.get_bins(V, block)
        t = np.zeros(V, np.uint8)
        for w, b in w2b.items():
            t[int(w)] = b
        tables[f"bins_{V}_{block}"] = t
        np.random.seed(12345)
        assert (np.random.get_state()[1] == before).all()
        assert (bc.word2bin_table(V, block) == t).all()
        assert (np.random.get_state()[1] == before).all(), "the restated get_bins touched numpy's global generator"
    np.savez_compressed(HERE / "bb_get_bins.npz", **tables)
    print("done", flush=True)


if __name__ == "__main__":
    main()
