"""ov2_match_to_map_batch (Mapper::matchToMap for B frames, csrc/match.hip) against the checker (oracle.match_to_map, applied
per frame), EXACTLY on indices and distances: only integers and gate decisions come out.  tests/test_match_batch_cpu.py
asserts on the checker alone that the synth_match frames hold the effects these tests lean on."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import _lib, mapper, synth_match as SM
from ov2slam_amd.ba_types import CamModelC

pytestmark = pytest.mark.gpu
GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)


@pytest.fixture(scope="module")
def frames():
    return SM.make_frames()


@pytest.fixture(scope="module")
def expected(oracle, frames):
    return {name: oracle.match_to_map(SM.single_input(f), *GATES) for name, f in frames.items()}


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_all_frames_in_one_call(ctx, frames, expected):
    inp = SM.batch_input(list(frames.values()))
    got = inp.split(*mapper.matchToMap_batch(ctx, inp, *GATES))
    for name, g in zip(frames, got):
        assert _same(g, expected[name]), name
    assert sum(int((mc >= 0).sum()) for mc, _ in got) > 20 * 6


@pytest.mark.parametrize("name", ["plain_a", "few3d", "no_kp", "borders", "no_cand", "short_kf", "dense", "plain_b"])
def test_frame_alone_is_its_slot_and_the_single_call(ctx, frames, expected, name):
    f = frames[name]
    one = SM.batch_input([f])
    mc, md = mapper.matchToMap_batch(ctx, one, *GATES)
    assert _same((mc, md), expected[name])
    assert _same(mapper.matchToMap(ctx, SM.single_input(f), *GATES), (mc, md))


@pytest.mark.parametrize("comp", ["reversed", "empty_first", "empty_middle", "empty_last"])
def test_batch_composition_and_order(ctx, frames, expected, comp):
    names = SM.batches(frames)[comp]
    inp = SM.batch_input([frames[n] for n in names])
    for n, g in zip(names, inp.split(*mapper.matchToMap_batch(ctx, inp, *GATES))):
        assert _same(g, expected[n]), n


def test_dense_cells_of_more_than_64_keypoints(ctx, oracle, frames):
    fr = [frames["dense"], frames["plain_a"]]
    inp = SM.batch_input(fr, cell=SM.CELL_DENSE)
    assert np.diff(inp.grid_ptr).max() > 64
    for f, g in zip(fr, inp.split(*mapper.matchToMap_batch(ctx, inp, *GATES))):
        assert _same(g, oracle.match_to_map(SM.single_input(f, cell=SM.CELL_DENSE), *GATES))
        assert (g[0] >= 0).sum() > 20


def test_dev_form_bytewise(ctx, frames):
    inp = SM.batch_input(list(frames.values()))
    mc, md = mapper.matchToMap_batch(ctx, inp, *GATES)
    dc, dd = mapper.matchToMap_batch_dev(ctx, inp, *GATES)
    assert mc.tobytes() == dc.tobytes() and md.tobytes() == dd.tobytes()
    # keypoints of a frame without candidates are written (-1, 0), not left as they were
    one = SM.batch_input([frames["no_cand"]])
    dc, dd = mapper.matchToMap_batch_dev(ctx, one, *GATES)
    assert (dc == -1).all() and (dd == 0).all() and len(dc) == len(frames["no_cand"]["kps"]) > 0


def test_other_gates_and_lens_model(ctx, oracle, frames):
    fr = [frames["plain_a"], frames["few3d"], frames["borders"], frames["plain_b"]]
    cam = CamModelC.make(SM.K4, "radtan", SM.RADTAN)
    for gates, cm in (((4.0, 0.35), None), (GATES, cam)):
        inp = SM.batch_input(fr, cam=cm)
        got = inp.split(*mapper.matchToMap_batch(ctx, inp, *gates))
        for f, g in zip(fr, got):
            assert _same(g, oracle.match_to_map(SM.single_input(f, cam=cm), *gates))
        assert sum(int((mc >= 0).sum()) for mc, _ in got) > 20


def test_single_call_dense_cells_gates_and_lens_model(ctx, oracle, frames):
    """ov2_match_to_map, the B = 1 case of the batch form, against the checker on the inputs of the two tests above"""
    assert np.diff(SM.single_input(frames["dense"], cell=SM.CELL_DENSE).grid_ptr).max() > 64
    for name in ("dense", "plain_a"):
        inp = SM.single_input(frames[name], cell=SM.CELL_DENSE)
        got = mapper.matchToMap(ctx, inp, *GATES)
        assert _same(got, oracle.match_to_map(inp, *GATES)), name
        assert (got[0] >= 0).sum() > 20, name
    cam = CamModelC.make(SM.K4, "radtan", SM.RADTAN)
    for gates, cm in (((4.0, 0.35), None), (GATES, cam)):
        n = 0
        for name in ("plain_a", "few3d", "borders", "plain_b"):
            inp = SM.single_input(frames[name], cam=cm)
            got = mapper.matchToMap(ctx, inp, *gates)
            assert _same(got, oracle.match_to_map(inp, *gates)), (name, gates)
            n += int((got[0] >= 0).sum())
        assert n > 20


def test_single_call_without_pose_table(ctx, oracle, frames):
    """n_kf = 0 and kf_Twc = NULL with keyframe ids in the lists: every id is skipped, 0 / 0 compares false"""
    f = dict(frames["plain_a"], kf_Twc=np.zeros((0, 7)))
    inp = SM.single_input(f)
    inp.c.kf_Twc = None
    assert inp.c.n_kf == 0 and len(inp.kp_kfids) > 0
    exp = oracle.match_to_map(inp, *GATES)
    assert (exp[0] >= 0).sum() > 20
    assert _same(mapper.matchToMap(ctx, inp, *GATES), exp)


def test_single_call_refuses_what_the_batch_form_refuses(ctx, frames):
    """host-side refusals: nothing is launched for the bad inputs, the outputs keep the caller's values or the (-1, 0) pre-fill"""
    def call(edit):
        inp = SM.single_input(frames["borders"])
        mc, md = np.full(inp.c.n_kp, -7, np.int32), np.full(inp.c.n_kp, -7, np.float32)   # no output is negative but -1
        edit(inp)
        return ctx.lib.ov2_match_to_map(ctx.h, C.addressof(inp.c), 2.0, 0.2, mc.ctypes.data, md.ctypes.data), mc, md

    def raise_above_successor(i):
        i.kp_desc_ptr[3] = i.kp_desc_ptr[4] + 1
    n_kp = len(frames["borders"]["kps"])
    st, mc, md = call(lambda i: None)
    assert st == 0 and (mc >= 0).sum() > 0 and not (mc == -7).any() and not (md == -7).any()
    for edit in (lambda i: i.grid_kp.__setitem__(0, n_kp), lambda i: i.grid_kp.__setitem__(0, -1), raise_above_successor,
                 lambda i: i.cand_kf_ptr.__setitem__(0, 1)):
        st, mc, md = call(edit)
        assert st == -1                                                       # OV2_ERR_INVALID
        assert ((mc == -7) & (md == -7) | (mc == -1) & (md == 0)).all()
    assert (mapper.matchToMap(ctx, SM.single_input(frames["plain_a"]), *GATES)[0] >= 0).sum() > 20   # the context still works


def test_empty_and_invalid_arguments(ctx, frames):
    lib, INVALID = ctx.lib, -1                                          # OV2_ERR_INVALID
    empty = SM.batch_input([])
    mc, md = mapper.matchToMap_batch(ctx, empty, *GATES)                 # B = 0
    assert len(mc) == 0
    assert lib.ov2_match_to_map_batch(ctx.h, C.addressof(empty.c), 2.0, 0.2, None, None) == 0
    both = SM.batch_input([frames["no_kp"], frames["no_cand"]])
    mc, md = mapper.matchToMap_batch(ctx, both, *GATES)
    assert (mc == -1).all() and (md == 0).all() and len(mc) == len(frames["no_cand"]["kps"])

    def status(edit):
        inp = SM.batch_input([frames["borders"], frames["short_kf"]])
        out_c, out_d = np.zeros(inp.c.n_kp, np.int32), np.zeros(inp.c.n_kp, np.float32)
        edit(inp)
        return lib.ov2_match_to_map_batch(ctx.h, C.addressof(inp.c), 2.0, 0.2, out_c.ctypes.data, out_d.ctypes.data)

    assert status(lambda i: None) == 0
    assert status(lambda i: setattr(i.c, "B", -1)) == INVALID
    assert status(lambda i: setattr(i.c, "n_kp", -1)) == INVALID
    assert status(lambda i: setattr(i.c, "n_cand", -1)) == INVALID
    assert status(lambda i: setattr(i.c, "n_cand", i.c.n_cand + 1)) == INVALID      # does not span the offsets
    assert status(lambda i: setattr(i.c, "n_kp", i.c.n_kp - 1)) == INVALID
    assert status(lambda i: setattr(i.c, "cell", 0)) == INVALID
    for name, _ in mapper.BATCH_ARRAYS:
        assert status(lambda i: setattr(i.c, name, None)) == INVALID, name

    def edit_array(name, idx, value):
        def f(i):
            getattr(i, name)[idx] = value
        return f
    for off in ("kp_off", "cand_off", "kf_off"):
        assert status(edit_array(off, 0, 1)) == INVALID, off                       # does not start at 0
    assert status(lambda i: edit_array("kp_off", 1, i.kp_off[2] + 1)(i)) == INVALID     # frame 1 would have -1 keypoints
    assert status(lambda i: edit_array("cand_off", 1, i.cand_off[2] + 1)(i)) == INVALID
    assert status(lambda i: edit_array("kf_off", 1, i.kf_off[2] + 1)(i)) == INVALID
    assert status(lambda i: edit_array("kp_desc_ptr", 3, i.kp_desc_ptr[4] + 1)(i)) == INVALID   # a prefix array that decreases
    assert status(edit_array("grid_kp", 0, len(frames["borders"]["kps"]))) == INVALID           # one past frame 0's keypoints
    assert status(edit_array("grid_kp", 0, -1)) == INVALID
    inp = SM.batch_input([frames["borders"]])
    assert lib.ov2_match_to_map_batch(ctx.h, C.addressof(inp.c), 2.0, 0.2, None, None) == INVALID
    assert lib.ov2_match_to_map_batch(ctx.h, None, 2.0, 0.2, None, None) == INVALID
    assert lib.ov2_match_to_map_batch_dev(ctx.h, C.addressof(inp.c), 2.0, 0.2, None, None, None) == INVALID
    bad = SM.batch_input([frames["borders"]], cam=CamModelC.make(SM.K4, 7, (0.1,)))     # an unknown lens model
    with pytest.raises(_lib.Ov2Error):
        mapper.matchToMap_batch(ctx, bad, *GATES)
    # the context still works after the refusals
    ok = SM.batch_input([frames["plain_a"]])
    assert (mapper.matchToMap_batch(ctx, ok, *GATES)[0] >= 0).sum() > 20
