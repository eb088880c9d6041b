"""Host side of the rank coder's per-stream quality table (``ns_rank_stream_quality``): the row the kernels read, the
library's fill and its errors, the Python builder, and the call-shape validation of ``HipRankLM`` that runs before
any GPU work.  No device is needed: the fill is pure host arithmetic."""

from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from neuralsteganography_amd import _lib
from neuralsteganography_amd.exceptions import ConfigurationError
from tests import rank_vocab_cases as rv

ROOT = Path(__file__).resolve().parents[1]
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="libnsgcoder.so is not built")
POLICIES = rv.policies(4097)


def _fill(temp, quality):
    from neuralsteganography_amd.coder import rank_quality

    rq = quality if isinstance(quality, _lib.NsRankQuality) else rank_quality(quality)
    row = _lib.NsRankStreamQuality()
    rc = _lib.lib().ns_rank_stream_quality_fill(float(temp), ctypes.byref(rq), ctypes.byref(row))
    return rc, row


def test_struct_size_matches_the_header():
    text = (ROOT / "include" / "nsg_coder.h").read_text()
    size = int(re.search(r"#define NS_RANK_STREAM_QUALITY_BYTES (\d+)", text).group(1))
    assert size == _lib.NS_RANK_STREAM_QUALITY_BYTES == ctypes.sizeof(_lib.NsRankStreamQuality) == 48
    assert size % 8 == 0
    offsets = {n: getattr(_lib.NsRankStreamQuality, n).offset for n, _ in _lib.NsRankStreamQuality._fields_}
    assert offsets == {"inv_temp": 0, "top_p": 8, "min_prob": 16, "ptemp": 24, "c32": 32, "top_k": 36,
                       "cap_bits": 40, "crypto": 44}
    for name, off in offsets.items():  # the header documents every offset
        assert re.search(rf"{name};\s*/\*\s*{off}:", text), name


@needs_lib
def test_version_is_bumped_within_0_31():
    assert _lib.version().startswith("nsgcoder 0.31.") and _lib.version() != "nsgcoder 0.31.4 gfx950"


@needs_lib
def test_twelve_policies():
    assert len(POLICIES) == 12


@needs_lib
@pytest.mark.parametrize("name,quality,temp,scale", POLICIES, ids=[p[0] for p in POLICIES])
def test_fill_row_fields(name, quality, temp, scale):
    rc, row = _fill(temp, quality)
    assert rc == _lib.NS_OK
    inv = 1.0 / temp  # the host expression of the scalar entries' prepare()
    assert row.inv_temp == inv
    assert row.c32 == np.float32(inv * 1.4426950408889634)
    assert row.top_k == int(quality.get("top_k", 0))
    assert row.cap_bits == int(quality.get("cap_per_token_bits", 0))
    assert row.top_p == float(quality.get("top_p", 0.0))
    assert row.min_prob == float(quality.get("min_prob", -1.0))
    pt = float(quality.get("prob_temp", 0.0))
    assert row.crypto == (1 if pt > 0 else 0)
    # crypto/quality.py: the temperature step runs unless math.isclose(T, 1.0); crypto stays on either way
    assert row.ptemp == (pt if pt > 0 and not math.isclose(pt, 1.0) else 0.0)


@needs_lib
def test_isclose_rule_keeps_ptemp_and_crypto_distinct():
    for pt, want in ((1.0, 0.0), (1.0 + 5e-10, 0.0), (1.0 - 5e-10, 0.0), (1.0 + 2e-9, 1.0 + 2e-9), (0.999, 0.999)):
        rc, row = _fill(1.0, _lib.NsRankQuality(0, 0, 0.0, -1.0, pt))
        assert rc == _lib.NS_OK and row.crypto == 1 and row.ptemp == want, pt
        assert (want == 0.0) == math.isclose(pt, 1.0)


@needs_lib
@pytest.mark.parametrize("temp,rq", [
    (1.0, _lib.NsRankQuality(0, 0, 1.5, -1.0, 0.0)),              # top_p > 1
    (1.0, _lib.NsRankQuality(0, 3, 0.0, -1.0, 0.7)),              # prob_temp with a cap
    (1.0, _lib.NsRankQuality(0, 0, 0.0, 1e-6, 0.7)),              # prob_temp with min_prob
    (0.0, _lib.NsRankQuality(0, 0, 0.0, -1.0, 0.0)),              # temp = 0
    (-1.0, _lib.NsRankQuality(0, 0, 0.0, -1.0, 0.0)),             # temp < 0
    (float("nan"), _lib.NsRankQuality(0, 0, 0.0, -1.0, 0.0)),     # not > 0
], ids=["top_p>1", "ptemp+cap", "ptemp+min_prob", "temp0", "temp<0", "temp-nan"])
def test_fill_refuses_what_the_scalar_step_refuses(temp, rq):
    rc, row = _fill(temp, rq)
    assert rc == _lib.NS_ERR_CONFIG
    assert bytes(row) == bytes(48)  # nothing written


@needs_lib
def test_fill_null_arguments():
    row = _lib.NsRankStreamQuality()
    rq = _lib.NsRankQuality(0, 0, 0.0, -1.0, 0.0)
    L = _lib.lib()
    assert L.ns_rank_stream_quality_fill(1.0, None, ctypes.byref(row)) == _lib.NS_ERR_CONFIG
    assert L.ns_rank_stream_quality_fill(1.0, ctypes.byref(rq), None) == _lib.NS_ERR_CONFIG


@needs_lib
def test_builder_rows_are_the_library_rows():
    from neuralsteganography_amd.coder import RankStreamQuality, rank_stream_quality_rows

    quals = [dict(q, temp=t) for _, q, t, _ in POLICIES]
    rows = rank_stream_quality_rows(quals)
    assert rows.shape == (12, 6) and rows.dtype == np.int64
    for i, (_, q, t, _) in enumerate(POLICIES):
        assert rows[i].tobytes() == bytes(_fill(t, q)[1])
    # "temperature" is the other spelling, an explicit list overrides neither: both give the same rows
    assert np.array_equal(rank_stream_quality_rows([dict(q, temperature=t) for _, q, t, _ in POLICIES]), rows)
    assert np.array_equal(rank_stream_quality_rows([q for _, q, _, _ in POLICIES], [t for _, _, t, _ in POLICIES]),
                          rows)
    sq = RankStreamQuality(rows)
    assert len(sq) == 12 and np.array_equal(sq.take([3, 0]).rows, rows[[3, 0]])
    # the crypto provider's policy dict (crypto/arithmetic.py) is an element like any other
    assert rank_stream_quality_rows([{"prob_temp": 0.8, "top_k": 40, "top_p": 0.9}]).shape == (1, 6)


@needs_lib
@pytest.mark.parametrize("quality", [
    {"top_k": 0}, {"top_p": 0.0}, {"top_p": 1.5}, {"min_prob": -0.1}, {"cap_per_token_bits": 0}, {"prob_temp": 0.0},
    {"prob_temp": 0.7, "min_prob": 1e-6}, {"prob_temp": 0.7, "cap_per_token_bits": 3}, {"temp": 0.0},
    {"temperature": -1.0},
])
def test_builder_raises_what_rank_quality_raises(quality):
    from neuralsteganography_amd.coder import rank_quality, rank_stream_quality_rows

    with pytest.raises(ConfigurationError) as builder:
        rank_stream_quality_rows([{}, quality])
    if not {"temp", "temperature"} & set(quality):
        with pytest.raises(ConfigurationError) as single:
            rank_quality(quality)
        assert str(builder.value) == str(single.value)
    else:
        assert "temperature must be positive" in str(builder.value)


def _provider():
    """A provider object without a model or a device: the call-shape checks run before anything of it is used."""
    from neuralsteganography_amd.lm.rank import HipRankLM

    return object.__new__(HipRankLM)


def test_call_shape_is_validated_before_any_gpu_work():
    p = _provider()
    bits = [[0] * 8, [1] * 8]
    for entry in (p.encode_batch, p.encode_batch_states):
        with pytest.raises(ConfigurationError, match="exactly one of context"):
            entry(bits, quality={})
        with pytest.raises(ConfigurationError, match="exactly one of context"):
            entry(bits, [1, 2], contexts=[[1], [2]], quality={})
        with pytest.raises(ConfigurationError, match="exactly one of quality"):
            entry(bits, [1, 2])
        with pytest.raises(ConfigurationError, match="exactly one of quality"):
            entry(bits, [1, 2], quality={}, qualities=[{}, {}])
        with pytest.raises(ConfigurationError, match="3 contexts for 2 messages"):
            entry(bits, contexts=[[1], [2], [3]], quality={})
        with pytest.raises(ConfigurationError, match="1 qualities for 2 messages"):
            entry(bits, [1, 2], qualities=[{}])
    toks = [[5, 6], [7]]
    with pytest.raises(ConfigurationError, match="exactly one of context"):
        p.decode_batch(toks, quality={})
    with pytest.raises(ConfigurationError, match="exactly one of context"):
        p.decode_batch(toks, [1], contexts=[[1], [2]], quality={})
    with pytest.raises(ConfigurationError, match="exactly one of quality"):
        p.decode_batch(toks, [1])
    with pytest.raises(ConfigurationError, match="1 contexts for 2 messages"):
        p.decode_batch(toks, contexts=[[1]], quality={})
    with pytest.raises(ConfigurationError, match="3 qualities for 2 messages"):
        p.decode_batch(toks, [1], qualities=[{}, {}, {}])
    with pytest.raises(ConfigurationError, match="1 states for 2 messages"):
        p.decode_batch(toks, contexts=[[1], [2]], qualities=[{}, {}], states=[{}])


def test_front_end_finds_the_keywords():
    """``stego._takes`` routes ``seed_texts=`` / ``qualities=`` to a provider whose entries name them."""
    from neuralsteganography_amd import stego
    from neuralsteganography_amd.lm.rank import HipRankLM

    for entry in (HipRankLM.encode_batch, HipRankLM.decode_batch):
        assert stego._takes(entry, "contexts") and stego._takes(entry, "qualities")
