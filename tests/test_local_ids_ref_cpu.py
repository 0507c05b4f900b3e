"""The checker of the local-map selection (tests/local_ids_ref.py) against the C++ host stage -- MapManager::updateFrameCovisibility
and SlamManager::extendLocalMap on a host_map.LoopMap, no GPU -- on every case of tests/local_ids_cases.py, and every case
against the branch its name promises.  Sets are compared as sets: the host iterates a std::unordered_set."""
import pytest

import local_ids_cases as LC
from ov2slam_amd import host_map


@pytest.fixture(scope="module")
def cases():
    import __graft_entry__ as g
    g.build()
    return {c["name"]: c for c in LC.make_cases()}


NAMES = LC.NAMES


def host_stage(c):
    """the case on the host objects: stored sets, then the edits, then the two calls; (cov map, extended, ids)"""
    hm = host_map.LoopMap(c["scene"])
    for kf, ids in c["sets"].items():
        hm.set_local_ids(kf, ids)
    for e in c["edits"]:
        if e[0] == "remove_obs":
            hm.remove_obs(e[1], e[2])
        elif e[0] == "remove_keyframe":
            hm.remove_keyframe(e[1])
        elif e[0] == "remove_landmarks":
            for l in e[1]:
                hm.remove_landmark(l)
        else:
            raise ValueError(e[0])
    cov = hm.update_frame_covisibility(c["k"])
    extended = hm.extend_local_map(c["k"], c["nmax"]) if c["extend"] else False
    ids = hm.local_ids(c["k"])
    hm.close()
    return cov, extended, ids


def test_every_case_is_listed(cases):
    assert sorted(cases) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_checker_equals_the_host_stage(cases, name):
    c = cases[name]
    want = LC.expected(c)
    cov, extended, ids = host_stage(c)
    assert len(ids) == len(set(ids)) and set(ids) == set(want["lmid"])
    assert cov == dict(zip(want["cov_kfid"], want["cov_score"]))
    assert int(extended) == want["extended"]
    assert (min(cov) if cov else -1) == want["oldest_cov"]


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_branch(cases, name):
    c = cases[name]
    r = LC.expected(c)
    assert (r["swapped"], r["extended"]) == (c["swapped"], c["extended"])
    old = c["sets"].get(c["k"], [])
    assert r["swapped"] == int(2 * r["n_fresh"] > len(old))
    assert all(l not in r["lmid"] for l in c.get("absent", ())) and all(l in r["lmid"] for l in c.get("present", ()))
    assert r["lmid"] == sorted(set(r["lmid"]))


def test_the_named_edges_hold(cases):
    ex = {n: LC.expected(c) for n, c in cases.items()}
    nS = ex["plain_swap"]["n_fresh"]
    assert len(cases["union"]["sets"][LC.NEWKF]) > 2 * nS and 2 * ex["union"]["n_fresh"] <= len(cases["union"]["sets"][LC.NEWKF])
    assert len(cases["equality_edge"]["sets"][LC.NEWKF]) == 2 * ex["equality_edge"]["n_fresh"]
    assert len(cases["just_over_the_edge"]["sets"][LC.NEWKF]) == 2 * nS - 1
    assert set(ex["union"]["lmid"]) == set(ex["plain_swap"]["lmid"]) | set(cases["union"]["sets"][LC.NEWKF])
    taken, closed = ex["extend_taken"], ex["extend_gate_closed_at_count"]
    assert len(taken["lmid"]) > len(closed["lmid"]) == nS == cases["extend_gate_closed_at_count"]["nmax"]
    assert ex["extend_oldest_without_set"]["lmid"] == ex["plain_swap"]["lmid"]          # taken, and nothing to add
    assert ex["empty_C"]["cov_kfid"] == [] and ex["empty_C"]["oldest_cov"] == -1 and ex["empty_C"]["lmid"] == cases["empty_C"]["sets"][LC.NEWKF]
    gone = cases["covisible_keyframe_removed"]
    assert ex["covisible_keyframe_removed"]["oldest_cov"] == ex["plain_swap"]["cov_kfid"][1] and gone["edits"][-1][1] == ex["plain_swap"]["oldest_cov"]
    assert ex["S_empty"]["n_fresh"] == 0 and ex["S_empty"]["cov_kfid"] and ex["S_empty_nothing_stored"]["lmid"] == []
    assert ex["k_without_rows"]["cov_kfid"] == [] and ex["k_without_rows"]["n_fresh"] == 0
    assert ex["dead_row"]["n_fresh"] != nS and ex["removed_landmark"]["n_fresh"] == nS - 4
    assert ex["padded_ids"]["n_fresh"] == nS and max(ex["padded_ids"]["cov_kfid"]) >= 65 and ex["padded_ids"]["lmid"][-1] >= 2049
