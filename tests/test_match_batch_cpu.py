"""What the GPU tests of the batched local-map matcher (tests/test_match_batch_gpu.py, tests/test_match_local_maps_gpu.py) lean
on, checked without a GPU: the checker (oracle.match_to_map, pinned against numpy by tests/test_match.py) finds the planted
effects in the synth_match frames, mapper.MatchBatchInput lays frame b out as its own mapper.MatchInput, the batches straddle
workgroups, and the host mirror's assembling half offers the right keypoints and candidates."""
import numpy as np
import pytest

from ov2slam_amd import host_map, mapper, synth_match as SM, synth_revisit as SR

GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)


@pytest.fixture(scope="module")
def frames():
    return SM.make_frames()


def test_planted_effects_on_the_checker(oracle, frames):
    for seed in (1, 2, 3):
        fr = frames if seed == 1 else SM.make_frames(seed)
        for name, f in fr.items():
            cell = SM.CELL_DENSE if name == "dense" else SM.CELL
            mc, md = oracle.match_to_map(SM.single_input(f, cell=cell), *GATES)
            if f["kps"] and f["cands"]:
                assert (mc >= 0).sum() > 20, (seed, name)
            else:
                assert (mc == -1).all() and (md == 0).all() and len(mc) == len(f["kps"])
        # borders: the keypoints of the border cells find their planted candidates, the two on x = 0 / y = 0 among them
        mc = oracle.match_to_map(SM.single_input(fr["borders"]), *GATES)[0]
        print("borders: edge keypoints matched:", int((mc[:SM.N_EDGE] >= 0).sum()), "of", SM.N_EDGE)
        assert (mc[:SM.N_EDGE] >= 0).all(), seed   # 5 bits and under 2 px from their keypoint; unrelated descriptors lie past mindist
        # few3d: the doubled gate of nb3dkps < 30 decides at least 10 keypoints
        few = fr["few3d"]
        assert few["nb3dkps"] == 29
        a = oracle.match_to_map(SM.single_input(few, nb3dkps=29), *GATES)[0]
        b = oracle.match_to_map(SM.single_input(few, nb3dkps=30), *GATES)[0]
        print("few3d: keypoints that differ between nb3dkps 29 and 30:", int((a != b).sum()))
        assert (a != b).sum() >= 10, seed
        # dense at cell = 376: a cell with more than 64 keypoints (the 64-at-a-time walk loops)
        di = SM.single_input(fr["dense"], cell=SM.CELL_DENSE)
        assert len(di.grid_ptr) == 5 and np.diff(di.grid_ptr).max() > 64
        # short_kf: an id past the pose table on a keypoint that a candidate reaches (it is matched)
        sk = fr["short_kf"]
        mc = oracle.match_to_map(SM.single_input(sk), *GATES)[0]
        n_kf = len(sk["kf_Twc"])
        past = np.array([any(k >= n_kf for k in kp["kfids"]) for kp in sk["kps"]])
        allpast = np.array([len(kp["kfids"]) > 0 and all(k >= n_kf for k in kp["kfids"]) for kp in sk["kps"]])
        assert (past & (mc >= 0)).sum() >= 1, seed
        assert allpast.sum() >= 1


def test_batch_input_slices_are_the_single_inputs(frames):
    fr = list(frames.values())
    B = SM.batch_input(fr)
    assert B.c.B == len(fr) and B.c.n_kp == sum(len(f["kps"]) for f in fr) and B.c.n_cand == sum(len(f["cands"]) for f in fr)
    assert B.kp_off[0] == B.cand_off[0] == B.kf_off[0] == 0 and len(B.grid_ptr) == len(fr) * B.ncells + 1
    for b, f in enumerate(fr):
        S = SM.single_input(f)
        k0, k1, c0, c1, f0, f1 = B.kp_off[b], B.kp_off[b + 1], B.cand_off[b], B.cand_off[b + 1], B.kf_off[b], B.kf_off[b + 1]
        assert np.array_equal(B.Twc[b], np.asarray(f["Twc"])) and B.nb3dkps[b] == f["nb3dkps"] == S.c.nb3dkps
        assert np.array_equal(B.kp_px[k0:k1], S.kp_px) and np.array_equal(B.cand_wpt[c0:c1], S.cand_wpt)
        assert np.array_equal(B.kf_Twc[f0:f1], S.kf_Twc)
        for ptr, flat, sptr, sflat, lo, hi in ((B.kp_desc_ptr, B.kp_descs, S.kp_desc_ptr, S.kp_descs, k0, k1),
                                               (B.kp_kf_ptr, B.kp_kfids, S.kp_kf_ptr, S.kp_kfids, k0, k1),
                                               (B.kp_kf_ptr, B.kp_kf_px, S.kp_kf_ptr, S.kp_kf_px, k0, k1),
                                               (B.cand_desc_ptr, B.cand_descs, S.cand_desc_ptr, S.cand_descs, c0, c1),
                                               (B.cand_kf_ptr, B.cand_kfids, S.cand_kf_ptr, S.cand_kfids, c0, c1),
                                               (B.grid_ptr, B.grid_kp, S.grid_ptr, S.grid_kp, b * B.ncells, (b + 1) * B.ncells)):
            assert np.array_equal(ptr[lo:hi + 1] - ptr[lo], sptr)
            assert np.array_equal(flat[ptr[lo]:ptr[hi]], sflat)


def test_batches_straddle_workgroups(frames):
    W = mapper.MATCH_BATCH_WAVES
    for name, names in SM.batches(frames).items():
        off = np.cumsum([len(frames[n]["cands"]) for n in names])
        assert off[-1] % W != 0, name                    # the last workgroup is partly idle
        assert any(o % W for o in off[:-1]), name        # a frame boundary inside a workgroup
        # few3d sits between two frames whose gate is not doubled
        if "few3d" in names:
            i = names.index("few3d")
            assert frames[names[i - 1]]["nb3dkps"] >= 30 and frames[names[i + 1]]["nb3dkps"] >= 30 and i > 0


def test_assemble_only_hook():
    import __graft_entry__ as g
    g.build()
    s = SM.local_map_scenes((1,))[0]
    m = host_map.LoopMap(s)
    kp_lmid, cand_lmid = host_map.match_assemble(m, SR.NEWKF, s["local"])
    ro = s["roles"]
    # keypoints: every keypoint of the new keyframe, in grid order (cells row-major, insertion order within a cell)
    v = s["kps"][SR.NEWKF]
    nbw = int(np.ceil(np.float32(SR.W) / np.float32(SR.CELL)))
    cell = [int(np.floor(uv[1] / np.float32(SR.CELL))) * nbw + int(np.floor(uv[0] / np.float32(SR.CELL))) for uv in v["uv"]]
    assert sorted(kp_lmid) == sorted(v["lmid"].tolist())
    cells_of = dict(zip(v["lmid"].tolist(), cell))
    walked = [cells_of[l] for l in kp_lmid]
    assert walked == sorted(walked)
    # candidates: the local set without what the frame observes, what is gone, not 3D or without descriptor
    observed = set(v["lmid"].tolist())
    refused = observed | set(ro["gone"]) | set(ro["no_desc"]) | set(ro["not3d"])
    assert set(cand_lmid) == set(s["local"]) - refused and len(cand_lmid) == len(set(cand_lmid))
    assert set(ro["identity"]) <= observed and not set(ro["identity"]) & set(cand_lmid)
    assert set(ro["local"][:50]) <= set(cand_lmid)
    # an empty local set offers nothing
    assert host_map.match_assemble(m, SR.NEWKF, []) == ([], [])
    m.close()
