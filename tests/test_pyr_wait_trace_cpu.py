"""scripts/pyr_wait_trace.py on a hand-written kernel trace of 30 rows: five frames, every second one a keyframe (three
stereo calls = two complete keyframe periods), tracking kernels on hardware queue 1, pyramid builds on queue 2.  One
tracking call starts 2 us behind the end of the build it consumes (it waited for it), one 80 us behind; the idle sums,
the within-10-us count, the pairing of builds and calls and the queue sets are known by construction."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LUT = '"void (anonymous namespace)::clahe_lut_wave_kernel(unsigned char const*, int, int)"'
PD = '"void (anonymous namespace)::pyrdown2_kernel(ov2_pyr_view, int)"'
CMP = '"void (anonymous namespace)::klt_compact_kernel<9>(ov2_pyr_view, int)"'
ST1 = '"void (anonymous namespace)::klt_stage1_kernel<9, 3>(ov2_pyr_view, ov2_pyr_view)"'
EPI = '"(anonymous namespace)::epi_gate_kernel(float const*, int)"'

# (kernel, queue, start us, end us), in the order the frame loop enqueues them
ROWS = [
    (LUT, 2, 0, 10), (PD, 2, 10, 20),          # build 0: left pyramid of frame 0 (a keyframe; no tracking call consumes it)
    (LUT, 2, 20, 30), (PD, 2, 30, 40),         # build 1: right pyramid of frame 0
    (CMP, 1, 70, 80), (EPI, 1, 80, 200),       # stereo call 0, 30 us behind build 1: period 0 starts at 70
    (LUT, 2, 100, 150), (PD, 2, 150, 200),     # build 2: left pyramid of frame 1
    (CMP, 1, 202, 210), (ST1, 1, 210, 300),    # tracking call 1 starts 2 us behind build 2
    (LUT, 2, 200, 220), (PD, 2, 220, 240),     # build 3: left pyramid of frame 2
    (CMP, 1, 320, 330), (ST1, 1, 330, 400),    # tracking call 2 starts 80 us behind build 3, 20 us of queue idle in front
    (LUT, 2, 240, 250), (PD, 2, 250, 260),     # build 4: right pyramid of frame 2
    (CMP, 1, 400, 410), (EPI, 1, 410, 500),    # stereo call 3: period 1 starts at 400
    (LUT, 2, 260, 270), (PD, 2, 270, 280),     # build 5: left pyramid of frame 3
    (CMP, 1, 500, 510), (ST1, 1, 510, 600),    # tracking call 4
    (LUT, 2, 420, 430), (PD, 2, 430, 440),     # build 6: left pyramid of frame 4
    (CMP, 1, 600, 610), (ST1, 1, 610, 700),    # tracking call 5
    (LUT, 2, 440, 450), (PD, 2, 450, 460),     # build 7: right pyramid of frame 4
    (CMP, 1, 705, 710), (EPI, 1, 710, 800),    # stereo call 6: end of period 1
]
T0 = 5_000_000_000                             # the trace's clock does not start at zero


@pytest.fixture(scope="module")
def reader():
    spec = importlib.util.spec_from_file_location("pyr_wait_trace", os.path.join(ROOT, "scripts", "pyr_wait_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def trace(tmp_path):
    assert len(ROWS) == 30
    d = tmp_path / "kt" / "host" / "123"
    d.mkdir(parents=True)
    p = d / "123_kernel_trace.csv"
    with open(p, "w") as f:
        f.write('"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n')
        for k, (name, q, s, e) in enumerate(ROWS):
            f.write(f'"KERNEL_DISPATCH",1,{q},{k},{name},{T0 + 1000 * s},{T0 + 1000 * e}\n')
    return tmp_path / "kt"


def test_calls_builds_and_periods(reader, trace, capsys):
    path, rows = reader.load(str(trace))           # a directory: the reader finds the trace under it
    assert path.endswith("123_kernel_trace.csv") and len(rows) == 30
    calls, periods, notes = reader.analyse(rows)
    assert notes == []
    us = lambda ns: ns / 1000.0
    # seven calls, each paired with the build the loop made for it
    assert [c["stereo"] for c in calls] == [True, False, False, True, False, False, True]
    assert [c["build"] for c in calls] == [1, 2, 3, 4, 5, 6, 7]
    assert [us(c["build_end"] - T0) for c in calls] == [40, 200, 240, 260, 280, 440, 460]
    assert [us(c["gap"]) for c in calls] == [30, 2, 80, 140, 220, 160, 245]
    assert calls[0]["idle_before"] is None         # nothing ran on its queue before it
    assert [us(c["idle_before"]) for c in calls[1:]] == [2, 20, 0, 0, 0, 5]
    # two complete keyframe periods
    assert len(periods) == 2
    p0, p1 = periods
    assert (us(p0["period"]), us(p0["stereo"])) == (330, 130) and (us(p1["period"]), us(p1["stereo"])) == (305, 100)
    assert (us(p0["track_idle"]), us(p1["track_idle"])) == (22, 5)
    assert (us(p0["pyr_idle"]), us(p1["pyr_idle"])) == (150, 265)
    assert (us(p0["pyr_idle_in_stereo"]), us(p1["pyr_idle_in_stereo"])) == (30, 60)
    assert (p0["calls"], p0["near"]) == (3, 1) and (p1["calls"], p1["near"]) == (3, 0)
    for p in periods:
        assert p["queues"]["tracking"] == ["1"] and p["queues"]["pyramid"] == ["2"]
        assert set(p["queues"]) == {"tracking", "pyramid"}
    assert (us(p0["dur"]["tracking"]), us(p0["dur"]["pyramid"])) == (308, 180)
    assert (us(p1["dur"]["tracking"]), us(p1["dur"]["pyramid"])) == (300, 40)
    # the printed report carries the same figures
    reader.report(str(trace))
    out = capsys.readouterr().out
    assert "7 tracking / stereo calls, 2 complete keyframe periods" in out
    assert "track_idle 13.5" in out and "pyr_idle 207.5" in out and "within_10us 0.5" in out


def test_busy_is_a_union(reader):
    assert reader.busy_ns([(0, 10), (5, 20), (30, 40)], 0, 100) == 30
    assert reader.busy_ns([(0, 10), (5, 20), (30, 40)], 8, 35) == 17
    assert reader.busy_ns([], 0, 10) == 0


def test_a_missing_build_is_reported(reader, trace):
    _, rows = reader.load(str(trace))
    rows = [r for r in rows if not (r[2] == "clahe_lut_wave_kernel" and r[0] == T0 + 100_000) and
            not (r[2] == "pyrdown2_kernel" and r[0] == T0 + 150_000)]     # build 2 gone: the pairing by count slips
    _, _, notes = reader.analyse(rows)
    assert notes and "pairing by count" in notes[0]
