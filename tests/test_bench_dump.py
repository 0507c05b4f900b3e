"""CPU checks of bench.py --dump-outputs on stand-in buffers: file names, float dtypes, detector rows past a sequence's
count zeroed, maps concatenated in order, and the seeded row sample past the size cap."""
import os

import numpy as np

import bench


class _Buf:
    def __init__(self, a):
        self.a = np.asarray(a)

    def get(self):
        return self.a.copy()


class _Map:
    def __init__(self, nk, nl, s):
        self.t = dict(kf_pose=np.full((nk, 7), s, np.float64), kf_state=np.ones(nk, np.uint8),
                      lm_xyz=np.arange(3 * nl, dtype=np.float64).reshape(nl, 3) + s, lm_state=np.full(nl, 7, np.uint8))

    def download(self):
        return {k: v.copy() for k, v in self.t.items()}


def _workload(seqs=3, kps=5, cap=4):
    wl = bench.Workload.__new__(bench.Workload)
    rng = np.random.default_rng(0)
    wl.out_xy = _Buf(rng.uniform(0, 700, (seqs * kps, 2)).astype(np.float32))
    wl.out_st = _Buf(rng.integers(0, 2, seqs * kps).astype(np.uint8))
    wl.p3p = _Buf(np.zeros(seqs, np.int32))
    wl.d_det_nout = _Buf(np.array([0, 2, 4], np.int32)[:seqs])
    wl.d_det_out = _Buf(rng.uniform(1, 700, (seqs, cap, 2)).astype(np.float32))   # uninitialised past the counts
    wl.d_det_thresh = _Buf(np.full(seqs, 0.001))
    return wl


def _pipeline(sizes):
    ba = bench.BaPipeline.__new__(bench.BaPipeline)
    ba.maps = [[_Map(nk, nl, 10.0 * i) for i, (nk, nl) in enumerate(sizes)]]
    return ba


def test_dump_writes_float_arrays_of_the_last_step(tmp_path):
    wl = _workload()
    names = bench.dump_outputs(str(tmp_path), wl, _pipeline([(4, 6), (5, 3)]))
    assert set(names) == {f[:-4] for f in os.listdir(tmp_path)}
    for n in names:
        assert np.load(tmp_path / f"{n}.npy").dtype in (np.float32, np.float64), n
    assert np.array_equal(np.load(tmp_path / "frame_xy.npy"), wl.out_xy.a)
    corners = np.load(tmp_path / "kf_corners_xy.npy")
    assert np.array_equal(corners[1, 2:], np.zeros((2, 2))) and np.all(corners[0] == 0) and np.all(corners[2] > 0)
    assert np.load(tmp_path / "ba_lm_xyz.npy").shape == (9, 3)
    assert np.array_equal(np.load(tmp_path / "ba_map_sizes.npy"), [[4, 6], [5, 3]])
    assert np.load(tmp_path / "ba_kf_pose.npy")[4, 0] == 10.0


def test_dump_past_the_cap_keeps_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 200_000)
    ba = _pipeline([(2, 20000)])
    bench.dump_outputs(str(tmp_path / "a"), _workload(), ba)
    bench.dump_outputs(str(tmp_path / "b"), _workload(), ba)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 200_000 + 128 * len(os.listdir(tmp_path / "a"))   # .npy headers
    rows = np.load(tmp_path / "a" / "ba_lm_xyz_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 20000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "ba_lm_xyz.npy"), ba.maps[0][0].t["lm_xyz"][rows])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
