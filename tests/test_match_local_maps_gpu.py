"""SlamManager::matchToLocalMaps (host mirror): the re-matching of B new keyframes against their local maps with ONE
ov2_match_to_map_batch call, on three synth_revisit local-map scenes, against the same jobs run as one ov2_match_to_map call
each (the per-keyframe path).  tests/test_match_batch_cpu.py checks what the assembling half offers."""
import numpy as np
import pytest

from ov2slam_amd import host_map, synth_match as SM, synth_revisit as SR

pytestmark = pytest.mark.gpu
GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)


@pytest.fixture(scope="module")
def scenes():
    import __graft_entry__ as g
    g.build()
    return SM.local_map_scenes((1, 2, 3))


def _maps(scenes):
    return [host_map.LoopMap(s) for s in scenes]


def _close(maps):
    for m in maps:
        m.close()


def test_batched_stage_equals_single_calls(ctx, scenes):
    maps = _maps(scenes)
    kf, lo = [SR.NEWKF] * 3, [s["local"] for s in scenes]
    one, st1 = host_map.match_local_maps(ctx, maps, kf, lo, *GATES, single=True)
    bat, stb = host_map.match_local_maps(ctx, maps, kf, lo, *GATES)
    assert bat == one
    offered = [host_map.match_assemble(m, SR.NEWKF, l) for m, l in zip(maps, lo)]
    want = dict(jobs=3, match_jobs=3, n_kp=sum(len(k) for k, _ in offered), n_cand=sum(len(c) for _, c in offered))
    assert stb == dict(want, match_calls=1) and st1 == dict(want, match_calls=3)
    for s, pairs in zip(scenes, bat):
        assert len(pairs) > 20 and len(set(pairs) & s["true_pairs"]) > 20       # the planted revisit
        assert [p[0] for p in pairs] == sorted(p[0] for p in pairs)             # ascending previous lmid
        assert len(set(p[1] for p in pairs)) == len(pairs)
    # the jobs in another order: each map's pairs stay its own
    rev, _ = host_map.match_local_maps(ctx, maps[::-1], kf, lo[::-1], *GATES)
    assert rev == bat[::-1]
    _close(maps)


def test_merge_moves_the_observations(ctx, scenes):
    maps = _maps(scenes)
    kf, lo = [SR.NEWKF] * 3, [s["local"] for s in scenes]
    before = [{l: m.landmark(l)[1] for l in s["local"]} for m, s in zip(maps, scenes)]
    pairs, st = host_map.match_local_maps(ctx, maps, kf, lo, *GATES, merge=True)
    assert st["match_calls"] == 1
    for m, s, pr, nobs in zip(maps, scenes, pairs, before):
        assert len(pr) > 20
        kps = set(m.keypoint_order(SR.NEWKF))
        for prev, new in pr:
            assert m.landmark(prev)[0] is None                      # the keyframe's own map point is gone from the map
            assert m.landmark(new)[1] == nobs[new] + 1              # and the surviving one is now seen by the new keyframe
            assert new in kps and prev not in kps
    # nothing is left to match: the survivors are observed by the frame, so they are no candidates any more
    again, _ = host_map.match_local_maps(ctx, maps, kf, lo, *GATES)
    for pr0, pr1 in zip(pairs, again):
        assert not {p[1] for p in pr0} & {p[1] for p in pr1}
    _close(maps)


def test_empty_local_set_is_skipped(ctx, scenes):
    maps = _maps(scenes)
    kf = [SR.NEWKF] * 3
    full, _ = host_map.match_local_maps(ctx, maps, kf, [s["local"] for s in scenes], *GATES)
    pairs, st = host_map.match_local_maps(ctx, maps, kf, [scenes[0]["local"], [], scenes[2]["local"]], *GATES)
    assert pairs == [full[0], [], full[2]]
    assert (st["jobs"], st["match_jobs"], st["match_calls"]) == (3, 2, 1)
    # nothing to offer anywhere: no library call; no jobs at all
    only_observed = [int(l) for l in scenes[1]["kps"][SR.NEWKF]["lmid"]]       # every one is a keypoint of the frame: no candidate
    pairs, st = host_map.match_local_maps(ctx, maps[:2], kf[:2], [[], only_observed], *GATES)
    assert pairs == [[], []] and (st["jobs"], st["match_jobs"], st["n_kp"], st["n_cand"], st["match_calls"]) == (2, 0, 0, 0, 0)
    pairs, st = host_map.match_local_maps(ctx, [], [], [], *GATES)
    assert pairs == [] and st["jobs"] == 0 and st["match_calls"] == 0
    _close(maps)


def test_mixed_cameras_are_refused(ctx, scenes):
    other = dict(scenes[1], K4=np.asarray(scenes[1]["K4"]) * 1.01)
    maps = [host_map.LoopMap(scenes[0]), host_map.LoopMap(other)]
    kf, lo = [SR.NEWKF] * 2, [scenes[0]["local"], scenes[1]["local"]]
    with pytest.raises(RuntimeError, match="status -1"):                       # OV2_ERR_INVALID: the call takes one camera
        host_map.match_local_maps(ctx, maps, kf, lo, *GATES)
    with pytest.raises(RuntimeError, match="status -1"):                       # a keyframe that is not in its map
        host_map.match_local_maps(ctx, maps[:1], [SR.MISSING], lo[:1], *GATES)
    pairs, st = host_map.match_local_maps(ctx, maps[:1], kf[:1], lo[:1], *GATES)      # the maps are untouched by the refusals
    assert len(pairs[0]) > 20 and st["match_calls"] == 1
    _close(maps)
