"""A handle's launch tuners (decombinator_amd/csrc/dcrx_tune.h) launch by launch under a scripted clock, and the debug knobs'
reader (dcrx_debug_flags.h): the stand-alone host program of tests/host_tune, no GPU.  The sequences are those launch_v2 ran
inline before the tuners became operations on a slot."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PROG = os.path.join(HERE, "host_tune", "build", "tune_host")


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_tune")])
    return PROG


def _num(v):
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


def run(prog, mode, env=None, **kw):
    """One dict per simulated launch."""
    out = subprocess.run([prog, mode] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True,
                         env=env).stdout
    return [{k: _num(v) for k, v in (f.split("=") for f in line.split())} for line in out.splitlines()]


def col(trace, key):
    return [t[key] for t in trace]


# ---- rescue waves ----

def test_rescue_second_candidate_two_percent_faster(prog):
    t = run(prog, "rescue", t1=1.0, t2=0.98, script="eeeeee")
    assert col(t, "waves") == [4096, 4096, 3072, 3072, 3072, 3072]
    assert col(t, "timed") == [0, 1, 1, 0, 0, 0]
    assert col(t, "choice") == [0, 0, 0, 3072, 3072, 3072]      # settled by the fourth launch, which already runs on it
    assert col(t, "launches") == [1, 2, 3, 4, 4, 4]             # ... and the count stops there
    assert col(t, "waited") == [0] * 6
    assert col(t, "queried") == [0, 0, 0, 2, 0, 0]              # both stop events, once
    assert (t[3]["us0"], t[3]["us1"]) == (1000.0, 980.0) and (t[2]["us0"], t[2]["us1"]) == (0.0, 0.0)


def test_rescue_second_candidate_one_percent_faster(prog):
    t = run(prog, "rescue", t1=1.0, t2=0.99, script="eeeee")
    assert col(t, "waves") == [4096, 4096, 3072, 4096, 4096]
    assert col(t, "choice") == [0, 0, 0, 4096, 4096]
    assert (t[3]["us0"], t[3]["us1"]) == (1000.0, 990.0)


def test_rescue_samples_not_complete_until_the_seventh_launch(prog):
    t = run(prog, "rescue", t1=1.0, t2=0.9, lag=4, script="eeeeeeee")      # sample 1 (launch 2) completes at launch 6
    assert col(t, "waves") == [4096, 4096, 3072, 4096, 4096, 4096, 3072, 3072]
    assert col(t, "choice") == [0, 0, 0, 0, 0, 0, 3072, 3072]
    assert col(t, "waited") == [0] * 8
    assert col(t, "launches") == [1, 2, 3, 4, 5, 6, 7, 7]
    assert col(t, "queried") == [0, 0, 0, 1, 1, 2, 2, 0]      # (a query that fails ends the round)


@pytest.mark.parametrize("may_wait", [0, 1])
def test_rescue_big_class_waits_once_and_only_with_permission(prog, may_wait):
    t = run(prog, "rescue", reads=1 << 25, t1=1.0, t2=0.9, lag=3, may_wait=may_wait, script="eeeeee")
    assert col(t, "waves")[:3] == [8192, 8192, 4096] and col(t, "timed") == [0, 1, 1, 0, 0, 0]
    if may_wait:
        assert col(t, "waited") == [0, 0, 0, 1, 0, 0]
        assert col(t, "choice") == [0, 0, 0, 4096, 4096, 4096] and col(t, "waves")[3:] == [4096] * 3
    else:
        assert col(t, "waited") == [0] * 6
        assert col(t, "choice") == [0, 0, 0, 0, 0, 4096] and col(t, "waves")[3:] == [8192, 8192, 4096]
    # below 2^25 reads the permission changes nothing
    s = run(prog, "rescue", reads=(1 << 25) - 1, lag=3, may_wait=1, script="eeeee")
    assert col(s, "waited") == [0] * 5 and col(s, "waves")[:3] == [4096, 4096, 3072]


@pytest.mark.parametrize("fail_create", [0, 3])
def test_rescue_event_creation_fails(prog, fail_create):
    t = run(prog, "rescue", t1=1.0, t2=0.5, fail_create=fail_create, script="eeee")
    assert col(t, "waves") == [4096] * 4 and col(t, "timed") == [0] * 4
    assert col(t, "choice") == [0, 4096, 4096, 4096]      # at once: by the launch that was to be the first sample
    assert col(t, "launches") == [1, 2, 2, 2] and col(t, "queried") == [0] * 4


def test_rescue_ineligible_launches_do_not_move_the_sample_index(prog):
    t = [x for x in run(prog, "rescue", t1=1.0, t2=0.98, script="eiieieiie") if x["class"] != "-"]
    assert col(t, "launch") == [0, 3, 5, 8]
    assert col(t, "waves") == [4096, 4096, 3072, 3072] and col(t, "timed") == [0, 1, 1, 0]
    assert col(t, "launches") == [1, 2, 3, 4] and t[3]["choice"] == 3072


def test_rescue_two_size_classes_on_one_handle(prog):
    t = run(prog, "rescue", reads=3000000, reads2=1500000, t1=1.0, t2=0.98, script="eEeEeEeE")
    a, b = [x for x in t if x["class"] == 1], [x for x in t if x["class"] == 0]
    for c in (a, b):
        assert col(c, "waves") == [4096, 4096, 3072, 3072] and col(c, "timed") == [0, 1, 1, 0]
        assert col(c, "launches") == [1, 2, 3, 4] and col(c, "choice") == [0, 0, 0, 3072]


# ---- list E inside the scan or a role ----

def test_list_e_share_above_the_limit(prog):
    t = run(prog, "liste", reads=3000000, entries=900000, script="f" * 20)
    assert col(t, "copies") == [1] + [0] * 19          # the first launch's counts, once
    assert col(t, "state") == [-1] + [0] * 19 and abs(t[1]["share"] - 0.3) < 1e-6
    assert col(t, "fused") == [0] * 20 and col(t, "pair") == [-1] * 20 and col(t, "phase") == [0] * 20
    # the limit itself still allows it
    assert run(prog, "liste", reads=3000000, entries=750000, script="ff")[1]["state"] == -2


@pytest.mark.parametrize("t_fused,settles", [(0.98, 1), (0.99, 0)])
def test_list_e_phases(prog, t_fused, settles):
    t = run(prog, "liste", reads=3000000, entries=300000, t1=1.0, t2=t_fused, script="f" * 20)
    assert t[0]["state"] == -1 and t[0]["copies"] == 1
    e = t[1:]      # the eligible launches 0 .. of the phase sequence
    assert col(e, "pair")[:16] == [-1] * 8 + [0, 1, 2] + [-1] + [3, 4, 5] + [-1]
    assert col(e, "fused")[:15] == [0] * 11 + [1] * 4
    assert col(e, "state")[:15] == [-2] * 15 and col(e, "phase")[:15] == list(range(1, 16))
    assert col(e, "queried")[:16] == [1] + [0] * 14 + [6]      # the counts' event, then nothing until the six stops are read
    assert col(e, "state")[15:] == [settles] * 4 and col(e, "fused")[15:] == [settles] * 4
    assert (e[15]["us0"], e[15]["us1"]) == (1000.0, round(1000 * t_fused, 1)) and e[14]["us0"] == 0.0
    assert col(e, "copies") == [0] * 19


def test_list_e_fused_runs_on_while_its_samples_are_read(prog):
    t = run(prog, "liste", t1=1.0, t2=1.2, lag=3, script="f" * 22)
    assert t[3]["state"] == -2      # (the counts took three launches too)
    e = t[3:]
    assert col(e, "pair")[8:15] == [0, 1, 2, -1, 3, 4, 5]
    assert col(e, "fused")[15:] == [1, 1, 0, 0] and col(e, "state")[15:] == [-2, -2, 0, 0]


def test_list_e_caller_events_or_sink_do_not_advance_the_phase(prog):
    t = run(prog, "liste", script="ffbbfbf")
    assert col(t, "phase") == [0, 1, 1, 1, 2, 2, 3] and col(t, "fused") == [0] * 7
    # ... in the timed phases either: the pair waits for the next free launch
    script = "f" * 9 + "bfbf"
    t = run(prog, "liste", script=script)
    assert col(t, "pair")[9:] == [-1, 0, -1, 1] and col(t, "phase")[9:] == [8, 9, 9, 10]


def test_list_e_no_room_for_the_event_ring(prog):
    t = run(prog, "liste", t1=1.0, t2=0.5, room=0, script="f" * 16)
    assert col(t, "fused") == [0] * 16
    assert col(t, "state")[1:12] == [-2] * 11 and col(t, "state")[12:] == [0] * 4      # the first launch that was to run fused


def test_list_e_counts_copy_fails(prog):
    t = run(prog, "liste", copy_ok=0, script="ffff")
    assert col(t, "copies") == [1, 0, 0, 0] and col(t, "state") == [0] * 4 and col(t, "fused") == [0] * 4
    t = run(prog, "liste", fail_create=0, script="ffff")      # the counts' event
    assert col(t, "state") == [0] * 4


def test_list_e_event_creation_fails(prog):
    t = run(prog, "liste", fail_create=5, script="ffff")      # (create 0: the counts' event)
    assert col(t, "state") == [-1, 0, 0, 0] and col(t, "fused") == [0] * 4 and col(t, "phase") == [0] * 4


def test_list_e_waits_for_the_rescue_choice(prog):
    t = run(prog, "liste", settle_at=6, script="f" * 10)
    assert col(t, "state") == [-1] + [-2] * 9
    assert col(t, "phase") == [0] * 6 + [1, 2, 3, 4]


# ---- the knobs' reader ----

def _knob(prog, value, lo, hi, fallback, flags="1"):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCRX_")}
    if flags is not None:
        env["DCRX_DEBUG_FLAGS"] = flags
    if value is not None:
        env["DCRX_DEBUG_TEST_KNOB"] = value
    return int(subprocess.run([prog, "knob", "DCRX_DEBUG_TEST_KNOB", str(lo), str(hi), str(fallback)], check=True,
                              capture_output=True, text=True, env=env).stdout)


def test_knob_reader(prog):
    assert _knob(prog, "5", 1, 8, 3) == 5
    assert _knob(prog, "1", 1, 8, 3) == 1 and _knob(prog, "8", 1, 8, 3) == 8
    assert _knob(prog, "0", 1, 8, 3) == 3 and _knob(prog, "9", 1, 8, 3) == 3 and _knob(prog, "-2", 1, 8, 3) == 3
    assert _knob(prog, "abc", 0, 8, -1) == -1 and _knob(prog, "", 0, 8, -1) == -1
    assert _knob(prog, None, 1, 8, 3) == 3
    assert _knob(prog, "99999999999999999999", 1, 2147483647, 3) == 3
    # only under DCRX_DEBUG_FLAGS=1
    assert _knob(prog, "5", 1, 8, 3, flags=None) == 3
    assert _knob(prog, "5", 1, 8, 3, flags="0") == 3
