"""Host side of the per-stream quality table (``ns_stream_quality``, library 0.31): the row layout the kernel reads,
and ``ns_stream_quality_fill`` -- pure host arithmetic, no device and no context.

The provider's ``qualities=`` argument validation needs a constructed provider, which needs a GPU: it lives in
``tests/test_gpu_stream_quality.py``.
"""

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from neuralsteganography_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "nsg_coder.h"
BANNED = [50256, 628]
C_TYPES = {"double": (ctypes.c_double, 8), "float": (ctypes.c_float, 4), "int32_t": (ctypes.c_int32, 4)}


def _fill(vocab, temp, topk, precision, k_max, banned=BANNED):
    row = _lib.NsStreamQuality()
    ban = (ctypes.c_int32 * max(1, len(banned)))(*banned)
    rc = _lib.lib().ns_stream_quality_fill(vocab, ban, len(banned), float(temp), topk, precision, k_max,
                                           ctypes.byref(row))
    return rc, row


def test_struct_layout_matches_the_header():
    text = HEADER.read_text()
    body = re.search(r"typedef struct ns_stream_quality \{(.*?)\} ns_stream_quality;", text, re.S).group(1)
    fields = re.findall(r"^\s*(double|float|int32_t)\s+(\w+);\s*/\*\s*(\d+):", body, re.M)
    assert [f[1] for f in fields] == [n for n, _ in _lib.NsStreamQuality._fields_]
    off = 0
    for ctype, name, stated in fields:
        py_type, size = C_TYPES[ctype]
        off = (off + size - 1) // size * size  # natural alignment, as the C compiler lays the struct out
        assert dict(_lib.NsStreamQuality._fields_)[name] is py_type, name
        assert getattr(_lib.NsStreamQuality, name).offset == off == int(stated), name
        off += size
    size = int(re.search(r"#define NS_STREAM_QUALITY_BYTES (\d+)", text).group(1))
    assert ctypes.sizeof(_lib.NsStreamQuality) == size == _lib.NS_STREAM_QUALITY_BYTES == (off + 7) // 8 * 8


def test_version_and_exports():
    assert _lib.version().startswith("nsgcoder 0.31")
    for name in ("ns_stream_quality_fill", "ns_set_stream_quality"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("vocab,banned,temp,topk,precision", [
    (50257, BANNED, 0.9, 300, 26), (50257, BANNED, 0.7, 2, 12), (50257, [], 1.3, 768, 40), (512, [511, 628], 1.0, 40, 16),
    (512, [511], 1.0, 600, 60), (700, [3, 3, 9, -1, 700], 0.5, 699, 1)])
def test_fill_derives_what_the_step_derives(vocab, banned, temp, topk, precision):
    rc, row = _fill(vocab, temp, topk, precision, max(topk, 700), banned)
    assert rc == _lib.NS_OK
    nvalid = vocab - len({b for b in banned if 0 <= b < vocab})
    assert (row.topk, row.K, row.precision, row.reserved) == (topk, min(topk, nvalid), precision, 0)
    assert row.inv_temp == 1.0 / temp
    assert row.c32 == np.float32(row.inv_temp * 1.4426950408889634)  # log2(e), as the scalar step computes it
    assert row.c32 == np.float32(row.inv_temp * math.log2(math.e))


def test_no_speculative_sample_below_two_sample_spacings():
    for topk in (2, 40, 300, 510):
        rc, row = _fill(512, 0.9, topk, 26, 510, [511, 628])
        assert rc == _lib.NS_OK and row.spec_j == 0


@pytest.mark.parametrize("dtype", [_lib.NS_DTYPE_F32, _lib.NS_DTYPE_F16])
def test_spec_j_grows_with_topk_up_to_the_single_pass_limit(dtype):
    limit = _lib.max_topk(dtype)
    assert limit in (768, 512)
    prev = 0
    for topk in range(1, limit + 1):
        rc, row = _fill(50257, 1.0, topk, 26, limit)
        assert rc == _lib.NS_OK
        assert 4 <= row.spec_j <= 160, (topk, row.spec_j)
        assert row.spec_j >= prev, (topk, row.spec_j, prev)
        prev = row.spec_j
    # the rule is a function of K alone: k_max only switches the sample on or off for the whole call
    assert _fill(50257, 1.0, 40, 26, 40)[1].spec_j == _fill(50257, 1.0, 40, 26, limit)[1].spec_j


def test_sample_off_at_k_max_is_off_in_every_row():
    """Where the rule gives no usable threshold at k_max (beyond 160), every row of that call gets 0: the sample is
    on for every row of a launch or for none."""
    k_off = next(k for k in range(768, 4000, 8) if _fill(50257, 1.0, k, 26, k)[1].spec_j == 0)
    assert _fill(50257, 1.0, 40, 26, k_off)[1].spec_j == 0
    assert _fill(50257, 1.0, 40, 26, 768)[1].spec_j > 0


@pytest.mark.parametrize("kw", [
    dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")), dict(topk=0), dict(topk=-3), dict(topk=301),
    dict(precision=0), dict(precision=61), dict(vocab=1), dict(vocab=3, banned=[0, 1]), dict(banned=list(range(9)))])
def test_fill_refuses_what_the_step_refuses(kw):
    a = dict(vocab=50257, temp=0.9, topk=300, precision=26, k_max=300, banned=BANNED)
    a.update(kw)
    rc, _ = _fill(a["vocab"], a["temp"], a["topk"], a["precision"], a["k_max"], a["banned"])
    assert rc == _lib.NS_ERR_CONFIG, kw
    assert _lib.lib().ns_last_error(None)


def test_fill_refuses_a_null_row():
    ban = (ctypes.c_int32 * 2)(*BANNED)
    assert _lib.lib().ns_stream_quality_fill(50257, ban, 2, 0.9, 300, 26, 300, None) == _lib.NS_ERR_CONFIG


def test_stream_quality_rows_are_the_filled_structs():
    from neuralsteganography_amd.coder import CoderParams, StreamQuality
    from neuralsteganography_amd.exceptions import ConfigurationError

    ps = [CoderParams(vocab=50257, temp=0.7, topk=40, precision=12), CoderParams(vocab=50257, temp=1.3, topk=300)]
    sq = StreamQuality(ps)
    assert sq.k_max == 300 and sq.max_precision == 26 and sq.rows.shape == (2, 4) and sq.rows.dtype == np.int64
    for i, p in enumerate(ps):
        _, row = _fill(50257, p.temp, p.topk, p.precision, 300)
        assert sq.rows[i].tobytes() == bytes(row)
    assert sq.take([1, 1, 0]).rows.tolist() == sq.rows[[1, 1, 0]].tolist()
    cp = sq.context_params()
    assert (cp.topk, cp.precision, cp.vocab) == (300, 26, 50257)
    with pytest.raises(ConfigurationError):
        StreamQuality(ps + [CoderParams(vocab=512, topk=40)])  # one vocabulary per call
    with pytest.raises(ConfigurationError):
        StreamQuality(ps, k_max=100)  # topk beyond k_max
    with pytest.raises(ConfigurationError):
        StreamQuality([])


def test_quality_groups_keep_one_mixed_group_and_one_per_wide_quality():
    from neuralsteganography_amd.coder import CoderParams
    from neuralsteganography_amd.lm.arithmetic import _quality_groups

    P = lambda k, t=1.0, p=16: CoderParams(vocab=512, temp=t, topk=k, precision=p)  # noqa: E731
    assert _quality_groups([P(40), P(300), P(512)], 512) == [[0, 1, 2]]
    assert _quality_groups([P(40), P(50000), P(300), P(50000), P(50000, 0.9)], 512) == [[0, 2], [1, 3], [4]]
    assert _quality_groups([P(600), P(600)], 512) == [[0, 1]]
