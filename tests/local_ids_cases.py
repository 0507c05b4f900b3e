"""The cases of the local-map selection tests (test_local_ids_ref_cpu.py, test_map_local_ids_gpu.py), each named by the branch it
takes.  They stand on synth_match.local_map_scenes: eleven keyframes, the new keyframe 60 sharing a dozen landmarks with the
keyframes around the loop candidate, about 300 landmarks.  Two things are put straight first, because host objects and mirror
only agree there: a landmark's keypoints carry ONE Keypoint::is3d_ in every keyframe (the mirror keeps the flag per landmark),
and the scene's forgotten landmarks are properly removed instead (a dangling lmid is a keypoint on the host and no live row in
the mirror).  A case = dict(name, scene, k, edits, sets, extend, nmax, swapped, extended, table): `edits` in the style of
map_match_ref (remove_obs / remove_keyframe / remove_landmarks), `sets` the stored sets {kfid: ids} before the call, `table` the
dump the checker works on (DeviceMap.download() layout), swapped / extended the branch the name promises.  Every choice below
is made on the checker (local_ids_ref) alone."""
import copy

import numpy as np

import local_ids_ref as R
from ov2slam_amd import synth_match as SM, synth_revisit as SR

NEWKF = SR.NEWKF
NMAX_BIG = 100000
NAMES = ["plain_swap", "union", "equality_edge", "just_over_the_edge", "extend_taken", "extend_taken_after_union",
         "extend_gate_closed_at_count", "extend_gate_open_below_count", "extend_oldest_without_set", "extend_not_asked", "empty_C",
         "covisible_keyframe_removed", "kp3d_decides_not_3d", "candidate_k_observes", "dead_row", "removed_landmark", "S_empty",
         "S_empty_nothing_stored", "k_without_rows", "padded_ids"]


def _first_flags(s):
    """lmid -> (kp3d, lm3d) of the first keyframe (ascending kfid) that sees it"""
    first = {}
    for k in sorted(s["kfids"]):
        v = s["kps"][k]
        lm3d = v.get("lm3d", v["kp3d"])
        for i, l in enumerate(v["lmid"].tolist()):
            first.setdefault(l, (int(v["kp3d"][i]), int(lm3d[i])))
    return first


def base_scene(seed=1):
    """(scene, edits): the seeded scene with one keypoint flag per landmark, and the removal of its forgotten landmarks"""
    s = copy.deepcopy(SM.local_map_scenes((seed,))[0])
    first = _first_flags(s)
    for k in s["kfids"]:
        v = s["kps"][k]
        v["kp3d"] = np.array([first[l][0] for l in v["lmid"].tolist()], np.uint8)
        v["lm3d"] = v["kp3d"].copy()
    gone = [int(l) for l in s["forget_lm"]]
    s["forget_lm"] = []
    return s, [("remove_landmarks", gone)]


def set_flags(s, lmid, kp3d, lm3d):
    """every keypoint of the landmark carries is3d_ = kp3d, the map point is 3D iff lm3d"""
    for k in s["kfids"]:
        v = s["kps"][k]
        sel = v["lmid"] == lmid
        v["kp3d"][sel] = kp3d
        v["lm3d"][sel] = lm3d


def relabel(s, kf_of, lm_of):
    """the same scene under other keyframe and landmark ids (both maps increasing)"""
    kps = {kf_of(k): dict(v, lmid=np.array([lm_of(l) for l in v["lmid"].tolist()], np.int32)) for k, v in s["kps"].items()}
    return dict(K4=s["K4"], w=s["w"], h=s["h"], cell=s["cell"], kfids=[kf_of(k) for k in s["kfids"]],
                poses={kf_of(k): p for k, p in s["poses"].items()}, kps=kps, desc={lm_of(l): d for l, d in s["desc"].items()},
                descs={lm_of(l): [(kf_of(q) if q in s["poses"] else q, d) for q, d in kd] for l, kd in s["descs"].items()},
                forget_lm=[], cov=[], pairs=dict(revisit=(kf_of(NEWKF), kf_of(SR.LC))), grid_kfs=[kf_of(NEWKF)])


def table_of(s, edits=()):
    """the dump of the scene's mirror (rows keyframe after keyframe in the order of s["kfids"], as DeviceMap.from_scene appends
    them) after the edits: dict(kf_state, lm_state, obs_kf, obs_lm, obs_flag)"""
    top = max(int(v["lmid"].max()) for v in s["kps"].values() if len(v["lmid"]))
    kf_state, lm_state = np.zeros(max(s["kfids"]) + 1, np.uint8), np.zeros(top + 1, np.uint8)
    kf_state[s["kfids"]] = 1
    for l, (kp3d, lm3d) in _first_flags(s).items():
        lm_state[l] = R.LM_ALIVE | R.LM_OBS | (R.LM_KP3D if kp3d else 0) | (R.LM_3D if lm3d else 0)
    obs_kf = np.concatenate([np.full(len(s["kps"][k]["lmid"]), k, np.int32) for k in s["kfids"]])
    obs_lm = np.concatenate([s["kps"][k]["lmid"] for k in s["kfids"]]).astype(np.int32)
    d = dict(kf_state=kf_state, lm_state=lm_state, obs_kf=obs_kf, obs_lm=obs_lm, obs_flag=np.ones(len(obs_kf), np.uint8))
    for e in edits:
        if e[0] == "remove_obs":
            d["obs_flag"][(obs_kf == e[1]) & (obs_lm == e[2])] = 0
        elif e[0] == "remove_keyframe":
            d["kf_state"][e[1]] = 0
        elif e[0] == "remove_landmarks":
            d["lm_state"][list(e[1])] = 0
        else:
            raise ValueError(e[0])
    return d


def _case(name, s, edits, sets, extend, nmax, swapped, extended, k=NEWKF, **extra):
    return dict(name=name, scene=s, k=k, edits=list(edits), sets={int(a): sorted(int(l) for l in b) for a, b in sets.items()},
                extend=bool(extend), nmax=int(nmax), swapped=int(swapped), extended=int(extended), table=table_of(s, edits), **extra)


def expected(c, sets=None):
    return R.local_ids(c["table"], c["sets"] if sets is None else sets, c["k"], c["extend"], c["nmax"])


def make_cases(seed=1):
    s, gone = base_scene(seed)
    base = R.local_ids(table_of(s, gone), {}, NEWKF, False, 0)
    S, C, nS = base["fresh"], base["cov_kfid"], base["n_fresh"]
    assert nS > 40 and len(C) >= 3
    ro = s["roles"]
    own = [int(l) for l in s["kps"][NEWKF]["lmid"]]
    outside = [int(l) for l in ro["outside"]]
    not_in_S = [l for l in outside if l not in S] + [9000 + i for i in range(4 * nS)]   # ids beyond the tables as well: they grow
    cases = []
    cases.append(_case("plain_swap", s, gone, {}, False, 0, 1, 0))
    # old holds more than 2 |S| ids, some of them in S: the union
    cases.append(_case("union", s, gone, {NEWKF: S[:7] + not_in_S[:2 * nS + 1 - 7]}, False, 0, 0, 0))
    cases.append(_case("equality_edge", s, gone, {NEWKF: S[:3] + not_in_S[:2 * nS - 3]}, False, 0, 0, 0))
    cases.append(_case("just_over_the_edge", s, gone, {NEWKF: S[:3] + not_in_S[:2 * nS - 4]}, False, 0, 1, 0))
    ext = S[5:15] + outside[:12] + own[:3]          # the oldest covisible keyframe's set: known ids, new ids, ids that k observes
    cases.append(_case("extend_taken", s, gone, {C[0]: ext, C[1]: outside[20:30]}, True, NMAX_BIG, 1, 1))
    cases.append(_case("extend_taken_after_union", s, gone, {NEWKF: not_in_S[:2 * nS + 9], C[0]: ext}, True, NMAX_BIG, 0, 1))
    cases.append(_case("extend_gate_closed_at_count", s, gone, {C[0]: ext}, True, nS, 1, 0))          # count == nmax_local
    cases.append(_case("extend_gate_open_below_count", s, gone, {C[0]: ext}, True, nS + 1, 1, 1))
    cases.append(_case("extend_oldest_without_set", s, gone, {C[1]: ext}, True, NMAX_BIG, 1, 1))
    cases.append(_case("extend_not_asked", s, gone, {C[0]: ext}, False, NMAX_BIG, 1, 0))
    shared = [int(l) for l in list(ro["identity"]) + list(ro["identity_in"])]
    cases.append(_case("empty_C", s, gone + [("remove_obs", NEWKF, l) for l in shared], {NEWKF: outside[:5], 15: ext}, True, NMAX_BIG, 0, 0))
    cases.append(_case("covisible_keyframe_removed", s, gone + [("remove_keyframe", C[0])], {C[0]: ext, C[1]: outside[:9]}, True, NMAX_BIG, 1, 1))
    # Keypoint::is3d_ decides, MapPoint::is3d_ does not: `a` (in S) keeps a 3D map point under 2D keypoints and leaves, `b` (a 2D
    # landmark of a covisible keyframe) gets 3D keypoints over a map point that is not 3D and enters
    s3 = copy.deepcopy(s)
    t0 = table_of(s, gone)
    kf0, lm0 = R.live_rows(t0)
    plain2d = sorted({int(l) for j, l in zip(kf0, lm0) if j in C and not t0["lm_state"][l] & R.LM_KP3D and l not in own})
    assert plain2d
    a, b = S[0], plain2d[0]
    set_flags(s3, a, 0, 1)
    set_flags(s3, b, 1, 0)
    cases.append(_case("kp3d_decides_not_3d", s3, gone, {}, False, 0, 1, 0, absent=[a], present=[b]))
    # a candidate that k observes: 3D keypoints in a covisible keyframe, never in the set -- not even from a stored set
    cases.append(_case("candidate_k_observes", s, gone, {}, False, 0, 1, 0, absent=shared))
    only = [l for l in S if (lm0 == l).sum() == 1][:3]                       # seen by one keyframe only: the row's death takes it out
    rows = [("remove_obs", int(kf0[lm0 == l][0]), l) for l in only]
    cases.append(_case("dead_row", s, gone + rows + [("remove_obs", NEWKF, shared[0])], {}, False, 0, 1, 0, absent=only))
    cases.append(_case("removed_landmark", s, gone + [("remove_landmarks", S[2:6] + shared[1:2])], {}, False, 0, 1, 0, absent=S[2:6]))
    s0 = copy.deepcopy(s)
    for l in set(int(x) for v in s0["kps"].values() for x in v["lmid"]):
        set_flags(s0, l, 0, 0)
    cases.append(_case("S_empty", s0, gone, {NEWKF: outside[:6], C[0]: ext}, True, NMAX_BIG, 0, 1))
    cases.append(_case("S_empty_nothing_stored", s0, gone, {}, False, 0, 0, 0))
    cases.append(_case("k_without_rows", s, gone + [("remove_obs", NEWKF, l) for l in own], {NEWKF: outside[:4]}, True, NMAX_BIG, 0, 0))
    # the same map under ids that cross the scan's 1024-wide blocks (lmids 2100 .. 3600) and the 64-keyframe wave step
    # (kfids 50 .. 100); the row count is not a multiple of 256
    kf_of, lm_of = (lambda k: k + 40), (lambda l: 2 * l + 1100)
    sp = relabel(s, kf_of, lm_of)
    gp = [("remove_landmarks", [lm_of(l) for l in gone[0][1]])]
    cp = _case("padded_ids", sp, gp, {kf_of(NEWKF): [lm_of(l) for l in outside[:8]], kf_of(C[0]): [lm_of(l) for l in ext]}, True, NMAX_BIG, 1, 1,
               k=kf_of(NEWKF))
    assert len(cp["table"]["obs_kf"]) % 256 and max(cp["scene"]["kfids"]) >= 65 and min(lm_of(l) for l in S) >= 2049
    cases.append(cp)
    return cases
