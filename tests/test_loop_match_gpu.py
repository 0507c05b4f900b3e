"""ov2_loop_match_to_map_batch (LoopCloser::matchToMap for B pairs, csrc/match.hip) against the checker
(tests/loop_verify_ref.py), EXACTLY on indices and distances: only integers and gate decisions come out, and
tests/test_loop_verify_ref_cpu.py asserts that no gate decision of these scenes is within rounding of its threshold."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import _lib, loop_match as LM, synth_revisit as SR
from ov2slam_amd.ba_types import CamModelC
import loop_verify_ref as LV

pytestmark = pytest.mark.gpu
CAMERA = (SR.K4, SR.W, SR.H, SR.CELL)
GATES = (SR.FMAXPROJERR, SR.FDISTRATIO)


@pytest.fixture(scope="module")
def pairs():
    return SR.make_match_pairs()


@pytest.fixture(scope="module")
def expected(pairs):
    return {name: LV.loop_match_to_map(p, *CAMERA, *GATES)[:2] for name, p in pairs.items()}


def _split(inp, mc, md):
    o = inp.kp_off
    return [(mc[o[b]:o[b + 1]], md[o[b]:o[b + 1]]) for b in range(len(o) - 1)]


def test_all_pairs_in_one_call(ctx, pairs, expected):
    inp = LM.LoopMatchInput(list(pairs.values()), *CAMERA)
    got = _split(inp, *LM.loopMatchToMap_batch(ctx, inp, *GATES))
    for name, (mc, md) in zip(pairs, got):
        assert np.array_equal(mc, expected[name][0]) and np.array_equal(md, expected[name][1]), name
    assert sum(int((mc >= 0).sum()) for mc, _ in got) > 80


@pytest.mark.parametrize("name", ["revisit_a", "dense", "no_kp", "borders", "masked", "no_cand", "revisit_b"])
def test_pair_alone_is_its_slot_in_the_batch(ctx, pairs, expected, name):
    inp = LM.LoopMatchInput([pairs[name]], *CAMERA)
    mc, md = LM.loopMatchToMap_batch(ctx, inp, *GATES)
    assert np.array_equal(mc, expected[name][0]) and np.array_equal(md, expected[name][1])


def test_batch_composition_and_order(ctx, pairs, expected):
    names = list(pairs)[::-1] + ["dense", "no_cand", "no_kp", "dense"]       # reversed, repeats, empty pairs at the end
    inp = LM.LoopMatchInput([pairs[n] for n in names], *CAMERA)
    for n, (mc, md) in zip(names, _split(inp, *LM.loopMatchToMap_batch(ctx, inp, *GATES))):
        assert np.array_equal(mc, expected[n][0]) and np.array_equal(md, expected[n][1]), n


def test_dev_form_bytewise(ctx, pairs):
    inp = LM.LoopMatchInput(list(pairs.values()), *CAMERA)
    mc, md = LM.loopMatchToMap_batch(ctx, inp, *GATES)
    dc, dd = LM.loopMatchToMap_batch_dev(ctx, inp, *GATES)
    assert mc.tobytes() == dc.tobytes() and md.tobytes() == dd.tobytes()
    # keypoints without candidates are written (-1, 0), not left as they were
    one = LM.LoopMatchInput([pairs["no_cand"]], *CAMERA)
    dc, dd = LM.loopMatchToMap_batch_dev(ctx, one, *GATES)
    assert (dc == -1).all() and (dd == 0).all() and len(dc) == len(pairs["no_cand"]["kps"])


def test_other_gates_and_lens_model(ctx, pairs):
    ps = [pairs["revisit_a"], pairs["borders"], pairs["dense"]]
    cam = CamModelC.make(SR.K4, "radtan", SR.RADTAN)
    for gates, cm, ref_cam in (((4.0, 0.2), None, None), (GATES, cam, SR.RADTAN)):
        inp = LM.LoopMatchInput(ps, *CAMERA, cam=cm)
        for p, (mc, md) in zip(ps, _split(inp, *LM.loopMatchToMap_batch(ctx, inp, *gates))):
            ec, ed, _ = LV.loop_match_to_map(p, *CAMERA, *gates, cam=ref_cam)
            assert np.array_equal(mc, ec) and np.array_equal(md, ed)


def test_empty_and_invalid_arguments(ctx, pairs):
    lib, INVALID = ctx.lib, -1                                          # OV2_ERR_INVALID
    empty = LM.LoopMatchInput([], *CAMERA)
    mc, md = LM.loopMatchToMap_batch(ctx, empty, *GATES)                 # B = 0
    assert len(mc) == 0
    assert lib.ov2_loop_match_to_map_batch(ctx.h, C.addressof(empty.c), 10.0, 0.3, None, None) == 0
    both = LM.LoopMatchInput([pairs["no_kp"], pairs["no_cand"]], *CAMERA)
    mc, md = LM.loopMatchToMap_batch(ctx, both, *GATES)
    assert (mc == -1).all() and (md == 0).all() and len(mc) == len(pairs["no_cand"]["kps"])

    def status(edit):
        inp = LM.LoopMatchInput([pairs["borders"], pairs["masked"]], *CAMERA)
        out_c, out_d = np.zeros(inp.c.n_kp, np.int32), np.zeros(inp.c.n_kp, np.float32)
        edit(inp)
        return lib.ov2_loop_match_to_map_batch(ctx.h, C.addressof(inp.c), 10.0, 0.3, out_c.ctypes.data, out_d.ctypes.data)

    assert status(lambda i: None) == 0
    assert status(lambda i: setattr(i.c, "B", -1)) == INVALID
    assert status(lambda i: setattr(i.c, "n_kp", -1)) == INVALID
    assert status(lambda i: setattr(i.c, "n_cand", i.c.n_cand + 1)) == INVALID      # does not span the offsets
    assert status(lambda i: setattr(i.c, "cell", 0)) == INVALID
    for name in ("Twc", "kp_off", "cand_off", "kp_px", "kp_matched", "kp_desc_ptr", "kp_descs", "kp_kf_ptr", "kp_kfids", "grid_ptr",
                 "grid_kp", "cand_wpt", "cand_desc_ptr", "cand_descs", "cand_kf_ptr", "cand_kfids"):
        assert status(lambda i: setattr(i.c, name, None)) == INVALID, name

    def negative_pair(i):
        i.kp_off[1] = i.kp_off[2] + 1                                              # pair 1 would have -1 keypoints
    assert status(negative_pair) == INVALID

    def grid_outside(i):
        i.grid_kp[0] = len(pairs["borders"]["kps"])                                # one past pair 0's keypoints
    assert status(grid_outside) == INVALID
    inp = LM.LoopMatchInput([pairs["borders"]], *CAMERA)
    assert lib.ov2_loop_match_to_map_batch(ctx.h, C.addressof(inp.c), 10.0, 0.3, None, None) == INVALID
    assert lib.ov2_loop_match_to_map_batch(ctx.h, None, 10.0, 0.3, None, None) == INVALID
    assert lib.ov2_loop_match_to_map_batch_dev(ctx.h, C.addressof(inp.c), 10.0, 0.3, None, None, None) == INVALID
    bad = LM.LoopMatchInput([pairs["borders"]], *CAMERA, cam=CamModelC.make(SR.K4, 7, (0.1,)))     # an unknown lens model
    with pytest.raises(_lib.Ov2Error):
        LM.loopMatchToMap_batch(ctx, bad, *GATES)
