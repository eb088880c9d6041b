"""CPU: the host side of per-message sampling (``sample_batch(contexts=, lengths=, temperatures=, topks=, seeds=)``):
the draw-key rule, the top-k grouping, the draw-row layout, the argument refusals raised before any device use, and
that the shared kernel cases discriminate -- under stream 0's parameters the oracle gives every other stream
different tokens, so a kernel that ignored the rows could not pass the GPU file."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from neuralsteganography_amd import _lib
from neuralsteganography_amd.exceptions import ConfigurationError
from neuralsteganography_amd.lm.arithmetic import (SAMPLE_SCHEDULE_KEYS, HipArithmeticLM, sample_draw_keys,
                                                   sample_plan, sample_topk_groups)
from tests import sample_stream_cases as sc

HEADER = Path(__file__).resolve().parents[1] / "include" / "nsg_coder.h"


def test_draw_row_layout_matches_header():
    text = HEADER.read_text()
    body = re.search(r"typedef struct ns_sample_draw \{(.*?)\} ns_sample_draw;", text, re.S).group(1)
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+)(?:\[\d+\])?;\s*/\*\s*(\d+):", body)}
    assert stated == {"seed": 0, "gid": 8, "length": 16, "reserved": 20}
    for name, off in stated.items():
        assert getattr(_lib.NsSampleDraw, name).offset == off, name
    size = int(re.search(r"#define NS_SAMPLE_DRAW_BYTES (\d+)", text).group(1))
    assert ctypes.sizeof(_lib.NsSampleDraw) == size == _lib.NS_SAMPLE_DRAW_BYTES == 32
    assert "ns_sample_step_streams" in _lib.EXPORTS


def test_draw_rows_are_the_struct_bytes():
    from neuralsteganography_amd.coder import sample_draw_rows

    seeds, gids, lens = [0, (1 << 64) - 1, (1 << 63) + 5, -1], [0, -3, 1 << 40, 7], [0, 1, 12, (1 << 31) - 1]
    rows = sample_draw_rows(seeds, gids, lens)
    assert rows.shape == (4, 4) and rows.dtype == np.int64
    for i in range(4):
        want = _lib.NsSampleDraw(seeds[i] & ((1 << 64) - 1), gids[i], lens[i], (ctypes.c_int32 * 3)(0, 0, 0))
        assert rows[i].tobytes() == bytes(want)
    for bad in ([-1], [1 << 31]):
        with pytest.raises(ConfigurationError):
            sample_draw_rows([1], [1], bad)
    with pytest.raises(ConfigurationError):
        sample_draw_rows([1, 2], [1], [1, 1])


def test_draw_key_rule():
    # one shared seed: today's rule, message i is stream stream_offset + i (a shard is an offset)
    assert sample_draw_keys(3, None, 42, 0) == ([42, 42, 42], [0, 1, 2])
    assert sample_draw_keys(3, None, 42, 10) == ([42, 42, 42], [10, 11, 12])
    # the all-scalar call is the special case: a shard of two at offset 1 continues the call of three
    full, part = sample_draw_keys(3, None, 7, 0), sample_draw_keys(2, None, 7, 1)
    assert [k[1:] for k in full] == [list(k) for k in part]
    # one seed per message: message i is sample(..., seed=seeds[i]) alone, i.e. draw id stream_offset
    assert sample_draw_keys(3, [5, 6, 7], 42, 0) == ([5, 6, 7], [0, 0, 0])
    assert sample_draw_keys(2, [5, 6], 42, 9) == ([5, 6], [9, 9])
    assert sample_draw_keys(0, None, 1, 0) == ([], [])
    with pytest.raises(ConfigurationError):
        sample_draw_keys(3, [1, 2], 0, 0)


def test_topk_grouping_has_at_most_two_groups():
    assert sample_topk_groups([40, 300, 512, 1], 512) == [[0, 1, 2, 3]]
    assert sample_topk_groups([40, 513, 300, 50000, -1, 0, 2000], 512) == [[0, 2], [1, 3, 4, 5, 6]]
    assert sample_topk_groups([-1, -1], 768) == [[0, 1]]  # every id is beyond the limit whatever the vocabulary
    assert sample_topk_groups([769, 768], 768) == [[1], [0]]
    assert sample_topk_groups([], 768) == []
    rng = np.random.default_rng(3)
    for _ in range(20):
        ks = rng.integers(-2, 3000, size=int(rng.integers(1, 40))).tolist()
        groups = sample_topk_groups(ks, 768)
        assert 1 <= len(groups) <= 2 and sorted(i for g in groups for i in g) == list(range(len(ks)))
        assert all(0 < ks[i] <= 768 for i in groups[0]) or len(groups) == 1
        assert all(g == sorted(g) for g in groups)  # the caller's order inside a group


def test_plan_defaults_and_refusals():
    assert sample_plan(3, 8, None, 0.9, None, 40, None) == ([8, 8, 8], [0.9, 0.9, 0.9], [40, 40, 40])
    assert sample_plan(2, 0, [3, 1], 1.0, [0.7, 1.3], -1, [2, -1]) == ([3, 1], [0.7, 1.3], [2, -1])
    for kw in (dict(lengths=[1, 2, 3]), dict(temperatures=[1.0]), dict(topks=[1, 2, 3, 4])):
        args = dict(lengths=None, temperatures=None, topks=None)
        args.update(kw)
        with pytest.raises(ConfigurationError):
            sample_plan(2, 4, args["lengths"], 1.0, args["temperatures"], 40, args["topks"])
    for bad in ([4, 0], [-1, 4]):
        with pytest.raises(ValueError):
            sample_plan(2, 4, bad, 1.0, None, 40, None)
    with pytest.raises(ValueError):
        sample_plan(2, 0, None, 1.0, None, 40, None)
    for bad in ([1.0, 0.0], [-0.5, 1.0], [float("nan"), 1.0]):
        with pytest.raises(ConfigurationError):
            sample_plan(2, 4, None, 1.0, bad, 40, None)
    with pytest.raises(ConfigurationError):
        sample_plan(2, 4, None, 0.0, None, 40, None)


class _NoDeviceLM:
    """A provider's LM that fails the test when anything reaches it."""

    native = True

    class shape:
        vocab = 512

    def __getattr__(self, name):
        raise AssertionError(f"the LM was reached ({name}) before the arguments were refused")


def _provider():
    import torch

    p = HipArithmeticLM.__new__(HipArithmeticLM)
    p._init(_NoDeviceLM(), None, torch.device("cpu"), "f16", None, 16)
    return p


def test_sample_batch_refuses_bad_arguments_before_any_device_use():
    p = _provider()
    c = [[1, 2], [3]]
    with pytest.raises(ConfigurationError):  # neither context nor contexts
        p.sample_batch(2, 4, lengths=[1, 2])
    with pytest.raises(ConfigurationError):
        p.sample_batch(2, 4)
    with pytest.raises(ConfigurationError):  # both
        p.sample_batch(2, 4, [1], contexts=c)
    with pytest.raises(ConfigurationError):  # one context per message
        p.sample_batch(3, 4, contexts=c)
    for kw in (dict(lengths=[1]), dict(temperatures=[1.0, 1.0, 1.0]), dict(topks=[40]), dict(seeds=[1, 2, 3])):
        with pytest.raises(ConfigurationError):
            p.sample_batch(2, 4, contexts=c, **kw)
    with pytest.raises(ValueError):
        p.sample_batch(2, 4, contexts=c, lengths=[4, 0])
    with pytest.raises(ValueError):
        p.sample_batch(2, 0, contexts=c)
    with pytest.raises(ConfigurationError):
        p.sample_batch(2, 4, contexts=c, temperatures=[1.0, 0.0])
    with pytest.raises(ConfigurationError):
        p.sample_batch(2, 4, contexts=c, temperature=-1.0)
    with pytest.raises(ConfigurationError):
        p.sample_batch(2, 4, contexts=c, slots=0)
    assert set(SAMPLE_SCHEDULE_KEYS) == {"slots", "quality_groups", "prefill_rows", "compactions", "evictions",
                                         "kv_pages_peak"}


def test_code_base_sample_batch_refusals():
    from neuralsteganography_amd import code_base

    p = _provider()
    with pytest.raises(ValueError):
        code_base.sample_batch(p, None, 0, [1, 2], 2)  # the unchanged scalar form
    with pytest.raises(ValueError):
        code_base.sample_batch(p, None, 4, None, 3, contexts=[[1], [2]])  # n must equal len(contexts)
    with pytest.raises(ValueError):
        code_base.sample_batch(p, None, 4, None, 2, contexts=[[1], [2]], lengths=[3, 0])
    with pytest.raises(ConfigurationError):
        code_base.sample_batch(p, None, 4, None, 2, contexts=[[1], [2]], temperatures=[1.0])


@pytest.mark.parametrize("name", list(sc.NAMES))
def test_cases_cover_what_they_claim_and_discriminate(name):
    case = sc.case(name)
    B = len(case.streams)
    assert B == 8 and max(s.length for s in case.streams) == sc.MAX_STEPS
    assert {s.length for s in case.streams} == {1, 5, 12}
    assert len({(s.seed, s.gid) for s in case.streams}) == B
    assert all(1 <= case.topk_of(s) <= case.k_max_row for s in range(B))
    lim = sc.limit(case.dtype)
    ks = {s.topk for s in case.streams}
    if name.startswith("single"):
        assert ks == {1, 2, 40, 100, 300, lim} and case.k_max == lim
        assert {s.temp for s in case.streams} == set(sc.TEMPS)
    if name == "wide_f32":
        assert ks == {lim + 1, 2000, sc.EVERY, 300} and case.k_max == sc.EVERY
    if name == "small_vocab":
        assert ks == {690, 2} and case.vocab < 2 * 4096  # no speculative sample below two sample spacings
    if name == "padded_stride":
        assert case.pad > 0
    ref = sc.reference(name)
    assert [len(t) for t, _ in ref] == [s.length for s in case.streams]
    # under stream 0's temperature, top-k, seed and draw id every other stream comes out differently
    differ = [sc.oracle_stream(case, s, like=0)[0] != ref[s][0] for s in range(1, B)]
    assert sum(differ) >= B - 1, differ


def test_provider_inputs_cover_what_they_claim():
    assert sc.CONTEXT_LENGTHS == (1, 31, 32, 33, 64, 65, 100) and len(sc.LENGTHS) == 7
    assert len(set(sc.PAIRS)) == 5 and len(set(sc.SEEDS)) == 7
    ctxs = sc.contexts()
    assert [len(c) for c in ctxs] == list(sc.CONTEXT_LENGTHS) and len({tuple(c) for c in ctxs}) == 7
