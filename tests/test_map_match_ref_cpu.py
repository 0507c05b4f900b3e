"""The numpy checker of the match gather (tests/map_match_ref.py) on its own, no GPU: its arrays, fed to the matcher's checker
(oracle.match_to_map), must find what synth_revisit.make_local_map_scene planted and refuse what the candidate filter of
Mapper::matchToMap refuses (src/mapper.cpp:613-624); observer lists stay ascending whatever the table order is.  The GPU tests
(tests/test_map_match_gpu.py) then hold the device gather to these arrays."""
import numpy as np
import pytest

import map_match_ref as R
from ov2slam_amd import synth_ba, synth_match as SM, synth_revisit as SR

GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def scenes():
    return SM.local_map_scenes(SEEDS)


def nb3d_of(s):
    return int(s["kps"][SR.NEWKF]["kp3d"].sum())


def frame_of(s, edits=(), max_kf=SR.NEWKF + 1):
    newkf, kp, cand = R.scene_lists(s)
    return R.Model(s).apply(edits).frame(newkf, kp, cand, nb3d_of(s), max_kf), kp, cand


def pairs_of(oracle, f, kp, cand):
    mc, _ = oracle.match_to_map(R.single_input(f), *GATES)
    return {kp[k]: cand[c] for k, c in enumerate(mc.tolist()) if c >= 0}


def test_scene_camera_is_the_matchers(scenes):
    s = scenes[0]
    assert np.array_equal(s["K4"], SM.K4) and (s["w"], s["h"], s["cell"]) == (SM.W, SM.H, SM.CELL)
    assert nb3d_of(s) >= 30   # the pixel gate is not doubled


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_planted_twins_are_matched(oracle, scenes, i):
    s = scenes[i]
    f, kp, cand = frame_of(s)
    pairs = pairs_of(oracle, f, kp, cand)
    twins = set(int(l) for l in s["roles"]["local"][:50])
    q_of = {l: q for q, l in s["true_pairs"] if l in twins}
    n_twins = {}
    for q, l in s["true_pairs"]:
        n_twins[q] = n_twins.get(q, 0) + 1
    alone = [l for l in sorted(twins) if n_twins[q_of[l]] == 1]   # (new_own[30:34] have a second twin among the `second` points)
    assert len(alone) == 46
    # Two of Mapper::matchToMap's gates refuse a true twin by geometry alone, and the scene does not plant around them: the
    # view-angle gate (cos of the larger half field of view, src/mapper.cpp:586-598, :640-645: it cuts the image corners) and
    # Frame::getSurroundingKeypoints (src/frame.cpp:624-650), which looks at the projection's cell and the cells above and to
    # the left only -- a keypoint just across the lower or right cell border is not seen.  Every other twin must be matched.
    T, K = np.asarray(s["Twc"]), SM.K4
    Rwc = synth_ba.quat_to_rot(T[3:])
    view_th = np.cos(np.arctan(max(np.float32(0.5 * SM.H / K[1]), np.float32(0.5 * SM.W / K[0]))))
    px_kp = {int(l): p for l, p in zip(s["kps"][SR.NEWKF]["lmid"], s["kps"][SR.NEWKF]["uv"])}
    due = []
    for l in alone:
        pc = (s["wpt"][l] - T[:3]) @ Rwc
        u, v = K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]
        cell_c, cell_r = int(np.floor(u / SM.CELL)), int(np.floor(v / SM.CELL))
        kc, kr = int(np.floor(px_kp[q_of[l]][0] / SM.CELL)), int(np.floor(px_kp[q_of[l]][1] / SM.CELL))
        if pc[2] / np.linalg.norm(pc) >= view_th and kc in (cell_c - 1, cell_c) and kr in (cell_r - 1, cell_r):
            due.append(l)
    assert len(due) >= 40
    for l in due:
        assert pairs.get(q_of[l]) == l, (l, q_of[l])


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_refused_candidates_never_match(oracle, scenes, i):
    s = scenes[i]
    f, kp, cand = frame_of(s)
    pairs = pairs_of(oracle, f, kp, cand)
    refused = set(int(l) for r in ("gone", "no_desc", "not3d", "identity", "identity_in") for l in s["roles"][r])
    assert refused <= set(cand) and not (set(pairs.values()) & refused)
    for c, l in enumerate(cand):   # they stay in the list, with two empty ranges
        if l in refused:
            assert len(f["cands"][c]["descs"]) == 0 and len(f["cands"][c]["kfids"]) == 0, l
    assert len(f["cands"]) == len(s["local"])
    assert sum(len(c["descs"]) > 0 for c in f["cands"]) > 100


def test_observer_lists_ascend_after_out_of_order_appends(oracle, scenes):
    s = scenes[0]
    newkf, kp, cand = R.scene_lists(s)
    base, _, _ = frame_of(s)
    pairs = pairs_of(oracle, base, kp, cand)
    q = sorted(pairs)[3]                      # a matched keypoint's landmark, first seen by the new keyframe
    l = int(s["roles"]["repeated"][0])        # a candidate seen from several keyframes
    rng = np.random.default_rng(5)
    old = [k for k in (15, 22) if k not in [int(kf) for kf in s["kfids"] if l in s["kps"][kf]["lmid"]]][0]
    px_q = s["kps"][newkf]["uv"][kp.index(q)]
    edits = [("append", 22, q, px_q + np.float32([0.5, -0.25]), rng.integers(0, 256, 32, dtype=np.uint8)),
             ("append", 15, q, px_q + np.float32([-0.5, 0.25]), None),
             ("append", old, l, np.float32([100, 100]), rng.integers(0, 256, 32, dtype=np.uint8))]
    f, _, _ = frame_of(s, edits)
    k = f["kps"][kp.index(q)]
    assert k["kfids"] == [15, 22, newkf] and len(k["descs"]) == 2      # table order is newkf, 22, 15
    assert np.array_equal(k["kf_px"][2], px_q) and np.array_equal(k["kf_px"][0], px_q + np.float32([-0.5, 0.25]))
    for e in f["kps"] + f["cands"]:
        assert list(e["kfids"]) == sorted(e["kfids"])
    c = f["cands"][cand.index(l)]
    assert old in c["kfids"] and len(c["kfids"]) == len(base["cands"][cand.index(l)]["kfids"]) + 1


def test_edits_change_what_is_listed(scenes):
    s = scenes[1]
    newkf, kp, cand = R.scene_lists(s)
    l = int(s["roles"]["local"][0])
    k0 = [int(k) for k in s["kfids"] if l in s["kps"][k]["lmid"]][0]
    base, _, _ = frame_of(s)
    assert len(base["cands"][cand.index(l)]["descs"]) >= 1
    for edits in ([("remove_obs", k0, l)], [("remove_keyframe", k0)], [("remove_landmarks", [l])]):
        f, _, _ = frame_of(s, edits)
        assert len(f["cands"][cand.index(l)]["descs"]) == 0 and len(f["cands"][cand.index(l)]["kfids"]) == 0
    # the conflict rule of a merge: new's row of the shared keyframe takes prev's descriptor only if it has none
    q = kp[0]
    d_prev = R.Model(s).desc[[i for i in range(len(R.Model(s).kf)) if R.Model(s).lm[i] == q][0]]
    for new_has, n_exp in ((False, True), (True, False)):
        d_new = np.full(32, 7, np.uint8)
        f, _, _ = frame_of(s, [("append", newkf, l, np.float32([50, 60]), d_new if new_has else None), ("merge", [(q, l)])])
        got = f["cands"][cand.index(l)]   # observed by the new keyframe now: refused as a candidate
        assert len(got["descs"]) == 0
        m = R.Model(s).apply([("append", newkf, l, np.float32([50, 60]), d_new if new_has else None), ("merge", [(q, l)])])
        descs = [m.desc[i].tobytes() for i in m.live_rows(l) if m.has[i]]
        assert (d_prev.tobytes() in descs) == n_exp
