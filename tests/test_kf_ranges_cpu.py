"""ov2_kf_ranges_independent (ov2slam_amd/csrc/ov2_internal.h through ctx.hip) through ctypes, no GPU: the byte-range rule
by which a tracking or stereo call may run beside a pending detector chain, and a detector chain beside a stereo call.
Nothing the call writes may meet what the chain reads or writes, nothing it reads may meet what the chain writes; two reads
of the same bytes are no conflict; ranges are half-open; an absent array (address 0) meets nothing."""
import ctypes as C

import pytest

from ov2slam_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _pairs(ranges):
    flat = [v for r in ranges for v in r]
    return (C.c_size_t * max(len(flat), 1))(*flat), len(ranges)


def _independent(lib, rd, wr, chain_rd, chain_wr):
    a, na = _pairs(rd)
    b, nb = _pairs(wr)
    c, nc = _pairs(chain_rd)
    d, nd = _pairs(chain_wr)
    return lib.ov2_kf_ranges_independent(a, na, b, nb, c, nc, d, nd)


CHAIN_RD = [(0x1000, 16), (0x2000, 384), (0x3000, 192), (0x4000, 48)]     # thresholds, keypoints, image indices, flags
CHAIN_WR = [(0x1000, 16), (0x5000, 8), (0x6000, 960)]                     # thresholds, counts, corners


def test_disjoint_arrays_are_independent(lib):
    rd = [(0x8000, 384), (0x9000, 384), (0xa000, 48), (0xb000, 192)]
    wr = [(0xc000, 384), (0xd000, 48), (0xe000, 8), (0xf000, 384)]
    assert _independent(lib, rd, wr, CHAIN_RD, CHAIN_WR) == 1


def test_reading_what_the_chain_reads_is_no_conflict(lib):
    assert _independent(lib, [(0x2000, 384), (0x4000, 48)], [(0xc000, 384)], CHAIN_RD, CHAIN_WR) == 1


@pytest.mark.parametrize("rd,wr", [
    ([(0x6000, 384)], []),                 # reads the corners the chain writes
    ([(0x1008, 8)], []),                   # reads a threshold the chain adapts
    ([], [(0x2000, 384)]),                 # writes the keypoints the chain reads
    ([], [(0x4000, 48)]),                  # writes the flags the chain reads
    ([], [(0x5004, 4)]),                   # writes a count the chain writes
    ([(0x8000, 8)], [(0x9000, 8), (0x63bf, 1)]),   # the last byte of the corner block
])
def test_every_kind_of_overlap_is_a_conflict(lib, rd, wr):
    assert _independent(lib, rd, wr, CHAIN_RD, CHAIN_WR) == 0


def test_ranges_are_half_open(lib):
    assert _independent(lib, [(0x63c0, 64)], [(0x1010, 16), (0x5008, 8), (0x5ff0, 16)], CHAIN_RD, CHAIN_WR) == 1
    assert _independent(lib, [(0x63bf, 64)], [], CHAIN_RD, CHAIN_WR) == 0
    assert _independent(lib, [], [(0x5ff0, 17)], CHAIN_RD, CHAIN_WR) == 0


def test_absent_and_empty_ranges_meet_nothing(lib):
    assert _independent(lib, [(0, 384)], [(0, 48)], CHAIN_RD, CHAIN_WR) == 1
    assert _independent(lib, [(0x6000, 384)], [], CHAIN_RD, [(0x1000, 16), (0x5000, 8), (0, 960)]) == 1
    assert _independent(lib, [(0x6000, 0)], [(0x2000, 0)], CHAIN_RD, CHAIN_WR) == 1
    assert _independent(lib, [], [], [], []) == 1


def test_the_rule_is_symmetric_in_the_two_calls(lib):
    """the detector's check against a stereo call (fork_at_stereo) and a tracking call's check against the chain are one
    rule with the roles swapped"""
    rd, wr = [(0x8000, 384), (0x6000, 8)], [(0xc000, 384)]
    assert _independent(lib, rd, wr, CHAIN_RD, CHAIN_WR) == _independent(lib, CHAIN_RD, CHAIN_WR, rd, wr) == 0
    rd = [(0x8000, 384)]
    assert _independent(lib, rd, wr, CHAIN_RD, CHAIN_WR) == _independent(lib, CHAIN_RD, CHAIN_WR, rd, wr) == 1


def test_bad_arguments(lib):
    a, _ = _pairs([(0x1000, 8)])
    assert lib.ov2_kf_ranges_independent(a, -1, a, 0, a, 0, a, 0) == -1
    assert lib.ov2_kf_ranges_independent(a, 17, a, 0, a, 0, a, 0) == -1
    assert lib.ov2_kf_ranges_independent(None, 1, a, 0, a, 0, a, 0) == -1
