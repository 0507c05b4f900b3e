"""The wait-packet column of scripts/pyr_wait_trace.py on the hand-written trace of tests/test_pyr_wait_trace_cpu.py: a
call issues one packet per build it is the first to consume (ov2_pyr_wait_ready waits once per build), so the stereo call
of the first frame, which no tracking call precedes, issues two (its own left pyramid and the right one) and every other
call one; with --every-wait (a library that waited for every pyramid a call reads) every call issues two.  The column is
derived from the pairing of calls and builds -- a kernel trace has no row for a packet -- so this checks the derivation;
what the library really issues is counted by ov2_ctx_pyr_wait_stats and asserted in tests/test_pyr_wait_elide_gpu.py."""
import test_pyr_wait_trace_cpu as T
from test_pyr_wait_trace_cpu import reader, trace  # noqa: F401  (fixtures)


def test_wait_packets_per_call(reader, trace, capsys):
    _, rows = reader.load(str(trace))
    calls, _, notes = reader.analyse(rows)
    assert notes == []
    assert [c["waits"] for c in calls] == [2, 1, 1, 1, 1, 1, 1]
    assert sum(c["waits"] for c in calls) == 8                 # the eight builds of the trace, each waited for once
    calls, _, _ = reader.analyse(rows, every_wait=True)
    assert [c["waits"] for c in calls] == [2] * 7
    reader.report(str(trace))
    out = capsys.readouterr().out
    assert "wait_packets" in out and "wait packets per call: 1.00" in out
    reader.report(str(trace), every_wait=True)
    assert "wait packets per call: 2.00" in capsys.readouterr().out


def test_a_trace_that_opens_with_a_tracking_call(reader, trace):
    """without the first stereo call the first tracking call is the first consumer of prev and of cur"""
    _, rows = reader.load(str(trace))
    rows = [r for r in rows if r[0] >= T.T0 + 100_000]         # drops builds 0 and 1 and stereo call 0
    calls, _, _ = reader.analyse(rows)
    assert [c["stereo"] for c in calls][:2] == [False, False]
    assert [c["waits"] for c in calls][:3] == [2, 1, 1]
