"""CPU: host logic of per-message contexts (one seed text per message, ``src/neuralstego/api.py:707-747``): the
block list and the prefill groups of the ragged prefill (``lm/gpt2.py``), a paged cache whose slots start at their
own lengths with no shared prefix (``lm/kvpages.py``), and the ``seed_texts`` keyword of the batched stego front end.
The device side is covered by ``tests/test_gpu_context_batch.py``."""

import numpy as np
import pytest
import torch

from neuralsteganography_amd.exceptions import ConfigurationError
from neuralsteganography_amd.lm.gpt2 import prefill_groups, ragged_blocks
from neuralsteganography_amd.lm.kvpages import PAGE_ROWS, KVPagePool, PagedKV
from neuralsteganography_amd.lm.mock import MockLM
from neuralsteganography_amd.stego import (stego_decode, stego_decode_batch, stego_encode, stego_encode_batch)


def test_block_list_of_ragged_sequences():
    lens = [1, 64, 65, 130, 17]
    seq_start, blocks = ragged_blocks(lens)
    assert seq_start.dtype == np.int32 and blocks.dtype == np.int32 and blocks.flags["C_CONTIGUOUS"]
    assert seq_start.tolist() == [0, 1, 65, 130, 260, 277]  # the cumulative sum
    want = {(s, b) for s, n in enumerate(lens) for b in range(-(-n // 64))}
    got = [tuple(r) for r in blocks.tolist()]
    assert len(got) == len(want) == 1 + 1 + 2 + 3 + 1 and set(got) == want  # every (sequence, block) exactly once
    idx = [b for _, b in got]
    assert idx == sorted(idx, reverse=True)  # longest first: block b visits b + 1 key blocks
    assert got[0] == (3, 2) and got[1:3] == [(2, 1), (3, 1)]
    with pytest.raises(ValueError):
        ragged_blocks([3, 0])
    with pytest.raises(ValueError):
        ragged_blocks([])


@pytest.mark.parametrize("budget", [1, 70, 130, 200, 10 ** 6])
def test_prefill_groups_are_whole_sequences_in_order_within_the_budget(budget):
    lens = [1, 31, 32, 33, 64, 65, 100, 7, 130, 2]
    groups = prefill_groups(lens, budget)
    assert [a for a, _ in groups] == [0] + [b for _, b in groups[:-1]] and groups[-1][1] == len(lens)  # a partition
    for a, b in groups:
        assert b > a
        rows = sum(lens[a:b])
        assert rows <= budget or b == a + 1  # only a sequence longer than the budget exceeds it, alone
        if b < len(lens):
            assert rows + lens[b] > budget  # greedy: the next sequence did not fit
    if budget >= sum(lens):
        assert groups == [(0, len(lens))]
    assert prefill_groups([], 10) == []


def _pool(budget_pages=None, seg_pages=4):
    holder = {}
    budget = None
    if budget_pages is not None:
        def budget():
            return (budget_pages - holder["pool"].total) * holder["pool"].page_bytes
    pool = KVPagePool(n_layer=2, n_head=2, head_dim=64, dtype=torch.float16, device="cpu", budget_bytes=budget,
                      seg_pages=seg_pages)
    holder["pool"] = pool
    return pool


def test_paged_cache_without_a_prefix_starts_slots_at_their_own_lengths():
    pool = _pool(seg_pages=4)
    kv = PagedKV(pool, 6, 0, 2)
    lens = np.array([1, 31, 32, 33, 100])
    slots = np.array([4, 0, 2, 5, 1])  # slot 3 stays empty
    kv.reset(slots, lens=lens)
    assert kv.lens_host[slots].tolist() == lens.tolist() and kv.lens[torch.from_numpy(slots)].tolist() == lens.tolist()
    assert kv.lens_host[3] == 0 and int(kv.lens[3]) == 0
    assert kv.ensure(slots, lens + 17).size == 0
    need = -(-(lens + 17) // PAGE_ROWS)
    assert kv.nch[slots].tolist() == need.tolist() == [1, 2, 2, 2, 4]
    assert kv.pages_in_use() == int(need.sum()) and kv.nch[3] == 0
    assert kv.width >= 4  # the table grew for the 100-row context
    tab = kv.table.numpy()
    mapped = tab[tab != 0]
    assert mapped.size == need.sum() and np.unique(mapped).size == mapped.size  # no page shared
    assert (kv.host == tab).all()
    # decode steps within the mapped pages: 32 * pages - length, per slot and for the set
    for s, n, p in zip(slots.tolist(), lens.tolist(), need.tolist()):
        assert kv.steps_reserved([s]) == 32 * p - n
    assert kv.steps_reserved(slots) == 28  # the 100-row slot: 128 - 100
    kv.advance(3)
    assert kv.steps_reserved(slots) == 25 and kv.lens_host[slots].tolist() == (lens + 3).tolist()
    # release gives the pages back and keeps the lengths; reset starts the slot over (length 0, or a new context)
    free0 = pool.free_pages
    kv.release([1])
    assert pool.free_pages == free0 + 4 and kv.nch[1] == 0 and not kv.table[1].any() and kv.lens_host[1] == 103
    kv.reset([1])
    assert kv.lens_host[1] == 0 and int(kv.lens[1]) == 0
    kv.reset([5, 2], lens=[40, 64])
    assert pool.free_pages == free0 + 8 and kv.lens_host[[5, 2]].tolist() == [40, 64]
    assert kv.lens[torch.tensor([5, 2])].tolist() == [40, 64]
    assert kv.ensure([5, 2], np.array([40, 64]) + 1).size == 0 and kv.nch[[5, 2]].tolist() == [2, 3]
    kv.set_lens([0], 5)
    assert kv.lens_host[0] == 5 and int(kv.lens[0]) == 5
    with pytest.raises(ValueError):
        PagedKV(pool, 2, 8, 2).reset([0], lens=[7])  # below the shared prefix


class _RecordingLM(MockLM):
    """MockLM that records the context of every packet it encodes / decodes."""

    def __init__(self):
        super().__init__()
        self.enc, self.dec = [], []

    def encode_arithmetic(self, bits, context, *, quality):
        self.enc.append((list(context), len(bits)))
        return super().encode_arithmetic(bits, context, quality=quality)

    def decode_arithmetic(self, tokens, context, *, quality):
        self.dec.append((list(context), len(list(tokens))))
        return super().decode_arithmetic(tokens, context, quality=quality)


def test_stego_batch_seed_texts_give_every_packet_its_owners_context():
    lm = _RecordingLM()
    msgs = [b"a" * 50, b"bb", bytes(range(70))]  # 3, 1 and 4 packets of 20 bytes
    seeds = ["first seed", "", "third"]
    res = stego_encode_batch(msgs, chunk_bytes=20, ecc="none", seed_texts=seeds, lm=lm)
    npk = [len(r) for r in res]
    assert npk == [3, 1, 4]
    want = [lm.encode_seed(seeds[i]) for i, n in enumerate(npk) for _ in range(n)]
    assert [c for c, _ in lm.enc] == want
    out = stego_decode_batch(res, ecc="none", seed_texts=seeds, lm=lm)
    assert out == msgs
    assert [c for c, _ in lm.dec] == want
    for i in range(3):  # each message also decodes alone with its own seed
        assert stego_decode(res[i], ecc="none", seed_text=seeds[i], lm=lm) == msgs[i]
    for bad in (seeds[:2], seeds + ["x"]):
        with pytest.raises(ConfigurationError):
            stego_encode_batch(msgs, chunk_bytes=20, ecc="none", seed_texts=bad, lm=lm)
        with pytest.raises(ConfigurationError):
            stego_decode_batch(res, ecc="none", seed_texts=bad, lm=lm)


def test_stego_batch_seed_text_alone_behaves_as_before():
    lm = _RecordingLM()
    msgs = [b"hello world", b"x" * 30]
    res = stego_encode_batch(msgs, chunk_bytes=16, ecc="none", seed_text="one seed", lm=lm)
    assert all(c == lm.encode_seed("one seed") for c, _ in lm.enc) and len(lm.enc) == 3
    assert stego_decode_batch(res, ecc="none", seed_text="one seed", lm=lm) == msgs
    assert all(c == lm.encode_seed("one seed") for c, _ in lm.dec) and len(lm.dec) == 3
    one = stego_encode(msgs[0], chunk_bytes=16, ecc="none", seed_text="one seed", lm=lm)
    assert stego_decode(one, ecc="none", seed_text="one seed", lm=lm) == msgs[0]


class _BatchLM(_RecordingLM):
    """A provider with batched entry points that take ``contexts=`` (the HipArithmeticLM signature)."""

    def encode_batch(self, bit_lists, context=None, *, contexts=None, quality):
        self.calls = getattr(self, "calls", []) + [("enc", context, contexts)]
        cs = contexts if contexts is not None else [context] * len(bit_lists)
        return [MockLM.encode_arithmetic(self, b, c, quality=quality) for b, c in zip(bit_lists, cs)]

    def decode_batch(self, token_lists, context=None, *, contexts=None, quality):
        self.calls = getattr(self, "calls", []) + [("dec", context, contexts)]
        cs = contexts if contexts is not None else [context] * len(token_lists)
        return [MockLM.decode_arithmetic(self, t, c, quality=quality) for t, c in zip(token_lists, cs)]


def test_stego_batch_seed_texts_reach_a_batched_provider_as_one_call():
    lm = _BatchLM()
    msgs = [b"a" * 50, b"bb"]
    seeds = ["s0", "s1"]
    res = stego_encode_batch(msgs, chunk_bytes=20, ecc="none", seed_texts=seeds, lm=lm)
    assert stego_decode_batch(res, ecc="none", seed_texts=seeds, lm=lm) == msgs
    c0, c1 = lm.encode_seed("s0"), lm.encode_seed("s1")
    assert lm.calls == [("enc", None, [c0, c0, c0, c1]), ("dec", None, [c0, c0, c0, c1])]
    lm.calls = []
    res = stego_encode_batch(msgs, chunk_bytes=20, ecc="none", seed_text="s0", lm=lm)
    assert lm.calls == [("enc", c0, None)]  # the shared call, as before


class _SharedOnlyBatchLM(_RecordingLM):
    """Batched entry points that take one shared context only (the rank coder's signature)."""

    def encode_batch(self, bit_lists, context, *, quality):
        raise AssertionError("a shared-context batch call cannot carry one context per packet")

    decode_batch = encode_batch


def test_stego_batch_seed_texts_drive_a_shared_only_provider_per_packet():
    lm = _SharedOnlyBatchLM()
    msgs = [b"a" * 30, b"bb"]
    seeds = ["s0", "s1"]
    res = stego_encode_batch(msgs, chunk_bytes=20, ecc="none", seed_texts=seeds, lm=lm)
    assert stego_decode_batch(res, ecc="none", seed_texts=seeds, lm=lm) == msgs
    c0, c1 = lm.encode_seed("s0"), lm.encode_seed("s1")
    assert [c for c, _ in lm.enc] == [c0, c0, c1] == [c for c, _ in lm.dec]
