"""CPU: the pure helpers of the chunked slot decoder (``lm/slots.py``) against hand-worked values, and the ``chunk``
validation of everything that can be built without a GPU."""

import numpy as np
import pytest

from neuralsteganography_amd.lm.slots import (MAX_CHUNK, SlotDecoder, check_chunk, chunk_counts, chunk_page_horizon,
                                              chunk_slots)


def test_counts_are_min_of_chunk_and_remaining():
    # fed, token count -> next iteration's tokens at C = 5
    fed = [0, 3, 10, 12, 13, 20, 0]
    nlen = [13, 13, 13, 13, 13, 13, 0]
    assert chunk_counts(fed, nlen, 5).tolist() == [5, 5, 3, 1, 0, 0, 0]  # 13 = 5 + 5 + 3; past the end: none
    assert chunk_counts(fed, nlen, 1).tolist() == [1, 1, 1, 1, 0, 0, 0]
    assert chunk_counts([7], [40], 16).tolist() == [16]
    # a whole message: the counts add up to its length and only the last differs from C
    fed, seen = 0, []
    while True:
        n = int(chunk_counts([fed], [37], 8)[0])
        if n == 0:
            break
        seen.append(n)
        fed += n
    assert seen == [8, 8, 8, 8, 5]


def test_slot_rule():
    # min(N, max(1, slots // C))
    assert chunk_slots(300, 64, 1) == 64
    assert chunk_slots(300, 64, 8) == 8
    assert chunk_slots(300, 64, 5) == 12
    assert chunk_slots(300, 3, 16) == 1  # fewer slots than the chunk: one slot
    assert chunk_slots(5, 64, 4) == 5  # never more slots than messages
    assert chunk_slots(12, 4096, 16) == 12
    assert chunk_slots(1, 1, 1) == 1
    for n, s, c in [(300, 64, 8), (300, 100, 16), (7, 9, 2), (40, 33, 5)]:
        assert chunk_slots(n, s, c) * c <= max(s, c)  # a forward has at most ``slots`` rows (or one slot's C)


def test_page_horizon():
    # check_every = 3 iterations of C = 4: 16 positions ahead, capped at the message's end
    assert chunk_page_horizon([10, 10, 100], [200, 20, 100], 3, 4).tolist() == [26, 20, 100]
    # chunk = 1 is the one-token rule: check_every + 1 positions
    assert chunk_page_horizon([10, 10], [200, 20], 16, 1).tolist() == [27, 20]
    assert chunk_page_horizon([0], [1000], 0, 16).tolist() == [16]
    # between two checks a slot moves at most check_every * C positions and the forward at the check itself
    # writes C more: everything it touches lies below the horizon
    lens, ce, c = 37, 4, 5
    assert lens + ce * c + c <= int(chunk_page_horizon([lens], [10 ** 6], ce, c)[0])


@pytest.mark.parametrize("bad", [0, -1, 17, 2.0, "4", None, True])
def test_chunk_outside_1_to_16_is_a_value_error(bad):
    with pytest.raises(ValueError):
        check_chunk(bad)


def test_chunk_bounds_accepted():
    assert MAX_CHUNK == 16
    assert [check_chunk(c) for c in (1, 2, 16, np.int64(5))] == [1, 2, 16, 5]


class _LM:
    def __init__(self, native=True, window=0):
        self.native, self.window = native, window


class _Provider:
    def __init__(self, lm):
        self.lm = lm


def test_slot_decoder_validates_chunk_without_a_gpu():
    lists = [[1, 2, 3]] * 6
    dec = SlotDecoder(_Provider(_LM()), None, lists, [0], slots=8, use_graph=False, chunk=4, check_every=3)
    assert dec.C == 4 and dec.S == 2 and dec.ahead == 16
    dec = SlotDecoder(_Provider(_LM()), None, lists, [0], slots=8, use_graph=False)
    assert dec.C == 1 and dec.S == 6 and dec.ahead == 17
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError):
            SlotDecoder(_Provider(_LM()), None, lists, [0], slots=8, use_graph=False, chunk=bad)
    with pytest.raises(ValueError):
        SlotDecoder(_Provider(_LM(native=False)), None, lists, [0], slots=8, use_graph=False, chunk=2)
    with pytest.raises(ValueError):
        SlotDecoder(_Provider(_LM(window=64)), None, lists, [0], slots=8, use_graph=False, chunk=2)
    # chunk = 1 is today's path: no such requirement
    SlotDecoder(_Provider(_LM(native=False)), None, lists, [0], slots=8, use_graph=False, chunk=1)


def test_stego_decode_batch_validates_chunk():
    from neuralsteganography_amd.stego import _chunk_kw

    class NoChunk:
        def decode_batch(self, spans, context, quality=None):
            return []

    class WithChunk:
        def decode_batch(self, spans, context, quality=None, chunk=1):
            return []

    assert _chunk_kw(NoChunk(), 1) == {} and _chunk_kw(WithChunk(), 1) == {}
    assert _chunk_kw(WithChunk(), 4) == {"chunk": 4}
    with pytest.raises(ValueError):
        _chunk_kw(NoChunk(), 4)
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            _chunk_kw(WithChunk(), bad)
