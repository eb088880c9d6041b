"""Host side of per-message coder quality on the wide path (``ns_set_stream_quality_wide``): the export and its
declaration, the front end's grouping with ``mix_wide=True`` (at most two groups: at or below the single-pass top-k
limit, and beyond it), and the rows ``StreamQuality`` holds for a ``k_max`` beyond the limit.  The kernels are checked
in ``tests/test_gpu_wide_stream_quality.py``.
"""

import ctypes
import re
from pathlib import Path

import numpy as np

from neuralsteganography_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "nsg_coder.h"
BANNED = [50256, 628]


def test_the_wide_entry_is_exported_and_declared():
    assert _lib.version().startswith("nsgcoder 0.31")
    assert "ns_set_stream_quality_wide" in _lib.EXPORTS and hasattr(_lib.lib(), "ns_set_stream_quality_wide")
    text = HEADER.read_text()
    assert re.search(r"\bint\s+ns_set_stream_quality_wide\s*\(\s*ns_ctx\s*\*\s*ctx\s*,\s*const\s+ns_stream_quality\s*\*"
                     r"\s*d_table\s*,\s*int\s+k_max\s*\)\s*;", text)
    # the narrow entry keeps its own declaration
    assert re.search(r"\bint\s+ns_set_stream_quality\s*\(", text)


def test_quality_groups_mix_the_wide_messages_into_one_group():
    from neuralsteganography_amd.coder import CoderParams
    from neuralsteganography_amd.lm.arithmetic import _quality_groups

    P = lambda k, t=1.0, p=16: CoderParams(vocab=512, temp=t, topk=k, precision=p)  # noqa: E731
    plist = [P(40), P(50000), P(300), P(50000), P(50000, 0.9)]
    assert _quality_groups(plist, 512, mix_wide=True) == [[0, 2], [1, 3, 4]]
    assert _quality_groups([P(600), P(50000, 0.9), P(60000, 1.0, 40)], 512, mix_wide=True) == [[0, 1, 2]]  # all wide
    assert _quality_groups([P(40), P(300, 0.7), P(512)], 512, mix_wide=True) == [[0, 1, 2]]  # all narrow
    # the two-argument call is what it was: one group per distinct quality beyond the limit
    assert _quality_groups(plist, 512) == [[0, 2], [1, 3], [4]]
    assert _quality_groups(plist, 512, False) == [[0, 2], [1, 3], [4]]


def test_the_provider_switch_defaults_to_one_wide_group():
    from neuralsteganography_amd.lm.arithmetic import HipArithmeticLM

    assert HipArithmeticLM.mix_wide_qualities is True


def test_stream_quality_rows_for_a_k_max_beyond_the_limit():
    from neuralsteganography_amd.coder import CoderParams, StreamQuality

    qs = [(50000, 1.0, 16), (60000, 1.0, 40), (2, 0.7, 12), (300, 0.9, 26), (5000, 1.3, 22)]
    for dtype in ("f32", "f16"):
        sq = StreamQuality([CoderParams(vocab=50257, precision=p, temp=t, topk=k, dtype=dtype) for k, t, p in qs])
        assert sq.k_max == 60000 and sq.max_precision == 40 and sq.rows.shape == (len(qs), 4)
        assert sq.context_params().topk == 60000
        ban = (ctypes.c_int32 * 2)(*BANNED)
        for i, (k, t, p) in enumerate(qs):
            row = _lib.NsStreamQuality()
            rc = _lib.lib().ns_stream_quality_fill(50257, ban, 2, float(t), k, p, 60000, ctypes.byref(row))
            assert rc == _lib.NS_OK
            assert sq.rows[i].tobytes() == bytes(row), (dtype, i)
            got = np.frombuffer(sq.rows[i].tobytes(), dtype=np.int32)
            assert got[3] == k and got[4] == min(k, 50255) and got[5] == p
            assert got[6] == 0 and row.spec_j == 0  # the sample is off at k_max, so it is off for every row
