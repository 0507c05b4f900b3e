"""ov2_cu_mask_build (ov2slam_amd/csrc/ctx.hip) through ctypes, no GPU: the CU mask of a share of n compute units out of
`total`, as (total + 31) // 32 uint32 words.  Bit k of a mask is compute unit k // 8 of XCD k % 8 (OV2_CU_MASK_XCDS,
include/ov2slam_hip.h), so XCD x of a device of `total` compute units owns the bits x, x + 8, ... below `total`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD, PACKED = 0, 1
NS = (1, 8, 31, 32, 33, 64, 255)
TOTALS = (256, 228)       # a whole number of compute units per XCD, and 28.5
SHARES = [(t, n) for t in TOTALS for n in NS if n < t]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ov2slam_amd import _lib
    return _lib.load()


def _xcds():
    txt = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    return int(re.search(r"#define\s+OV2_CU_MASK_XCDS\s+(\d+)", txt).group(1))


def _build(lib, total, n, layout):
    """(status, bits): the words unpacked into one bool per bit; two guard words behind the mask must stay untouched"""
    words = (total + 31) // 32
    buf = (C.c_uint32 * (words + 2))(*([0xa5a5a5a5] * (words + 2)))
    st = lib.ov2_cu_mask_build(total, n, layout, buf)
    arr = np.array(buf, np.uint32)
    assert (arr[words:] == 0xa5a5a5a5).all(), "the builder wrote past (total + 31) // 32 words"
    bits = ((arr[:words, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)
    return st, bits, arr[:words]


def _per_xcd(bits, xcds):
    return np.array([int(bits[x::xcds].sum()) for x in range(xcds)])


@pytest.mark.parametrize("layout", [SPREAD, PACKED])
@pytest.mark.parametrize("total,n", SHARES)
def test_popcount_and_range(lib, total, layout, n):
    st, bits, _ = _build(lib, total, n, layout)
    assert st == 0
    assert int(bits.sum()) == n
    assert not bits[total:].any(), "a bit at or past the total"


@pytest.mark.parametrize("total,n", SHARES)
def test_spread_is_even_over_the_xcds(lib, total, n):
    xcds = _xcds()
    _, bits, _ = _build(lib, total, n, SPREAD)
    cnt = _per_xcd(bits, xcds)
    assert cnt.sum() == n and cnt.max() - cnt.min() <= 1, cnt


@pytest.mark.parametrize("total,n", SHARES)
def test_packed_fills_xcds_in_order(lib, total, n):
    xcds = _xcds()
    _, bits, _ = _build(lib, total, n, PACKED)
    cnt = _per_xcd(bits, xcds)
    own = np.array([len(range(x, total, xcds)) for x in range(xcds)])     # compute units XCD x has
    left, want = n, []
    for x in range(xcds):
        want.append(min(left, own[x]))
        left -= want[-1]
    assert cnt.tolist() == want, (cnt, want)
    # inside the one XCD that is partly filled the low compute units come first
    for x in range(xcds):
        mine = bits[x::xcds][:own[x]]
        assert mine[:cnt[x]].all() and not mine[cnt[x]:].any()


def test_layouts_agree_where_they_must(lib):
    """one compute unit is bit 0 in both layouts; a whole XCD packed is every eighth bit"""
    xcds = _xcds()
    assert xcds == 8
    for layout in (SPREAD, PACKED):
        _, bits, words = _build(lib, 256, 1, layout)
        assert words[0] == 1 and not words[1:].any()
    _, _, words = _build(lib, 256, 32, PACKED)
    assert (words == 0x01010101).all()
    _, _, words = _build(lib, 256, 32, SPREAD)
    assert words[0] == 0xffffffff and not words[1:].any()


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("layout", [SPREAD, PACKED])
def test_refusals(lib, total, layout):
    for n in (0, -1, -256, total, total + 1, 10 * total):
        st, _, words = _build(lib, total, n, layout)
        assert st == -1, n                       # OV2_ERR_INVALID
        assert (words == 0xa5a5a5a5).all()       # and nothing written
    assert lib.ov2_cu_mask_build(total, 8, layout, None) == -1
    assert _build(lib, total, 8, 2)[0] == -1 and _build(lib, total, 8, -1)[0] == -1
    assert _build(lib, 0, 0, layout)[0] == -1
