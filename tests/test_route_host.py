"""The route of a decombine call (decombinator_amd/csrc/dcrx_route.h): which launches it consists of, from plain facts, through
the stand-alone host program of tests/host_route, no GPU.  The expected values are written from the rules, on both sides of
every boundary.  The program's defaults are a tag set like config 2's on uniform 150-nt reads (stride 40), 5 000 reads,
orientation reverse, no flags: the v2 kernels, the tail inside the scan through a ring of 16 batches.  Its scan block takes
57 856 bytes, the side tables 8 192, the buckets 2 048, a ring batch 3 840: 68 096 + 16 * 3 840 = 129 536 <= 163 840."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PROG = os.path.join(HERE, "host_route", "build", os.environ.get("DCRX_ROUTE_HOST", "route_host"))
KB = 1024
LDS_CU = 160 * KB


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_route")])
    return PROG


def route(prog, **kw):
    out = subprocess.run([prog] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout
    r = {}
    for f in out.split():
        k, v = f.split("=")
        r[k] = int(v) if v.lstrip("-").isdigit() else v
    return r


def is_fused_v2(r, ring=16):
    return (r["form"], r["last_form"], r["needs_tail_list"], r["passes"], r["frame0"], r["rpl0"], r["prefetch0"], r["ring0"]) == \
        ("v2", 2, 0, 1, 1, 2, 1, ring)


def is_v2_tail_outside(r, rpl=2, prefetch=1):
    return (r["form"], r["last_form"], r["needs_tail_list"], r["passes"], r["rpl0"], r["prefetch0"], r["ring0"]) == ("v2", 2, 1, 1, rpl, prefetch, 0)


def three(r):
    assert (r["form"], r["last_form"], r["needs_tail_list"], r["passes"]) == ("three", 1, 0, 0)
    return r["scan"], r["nw"], r["all_general"], r["rescue_kernel"], r["last"]


def test_defaults(prog):
    assert is_fused_v2(route(prog))
    r = route(prog, orientation="forward")
    assert (r["form"], r["frame0"], r["ring0"], r["needs_tail_list"]) == ("v2", 0, 16, 0)


def test_long_form_beyond_stride_128(prog):
    assert is_v2_tail_outside(route(prog, stride=128), rpl=1, prefetch=0)      # the longest register shape: one read per lane
    r = route(prog, stride=136)
    assert (r["form"], r["last_form"], r["needs_tail_list"], r["passes"]) == ("long", 0, 0, 0)
    assert route(prog, stride=136, orientation="both", flags="V1_KERNELS")["form"] == "long"


def test_ring_only_on_the_150_nt_shape(prog):
    assert is_fused_v2(route(prog, stride=40))
    assert is_v2_tail_outside(route(prog, stride=48), rpl=1)                    # default shape beyond 150 nt: one read per lane
    assert is_v2_tail_outside(route(prog, stride=48, flags="SHAPE2"), rpl=2)    # two per lane there: still no ring


@pytest.mark.parametrize("uniform", [1, 0])
def test_launch_shapes(prog, uniform):
    assert is_fused_v2(route(prog, uniform=uniform))
    assert is_fused_v2(route(prog, uniform=uniform, flags="SHAPE2"))
    assert is_v2_tail_outside(route(prog, uniform=uniform, flags="SHAPE3"), rpl=1)
    r = route(prog, uniform=uniform, flags="SHAPE1")      # four per lane: uniform batches on narrow tables only, else two
    assert is_v2_tail_outside(r, rpl=4, prefetch=0) if uniform else is_fused_v2(r)
    assert is_fused_v2(route(prog, uniform=uniform, flags="SHAPE1", narrow1=0))
    assert is_v2_tail_outside(route(prog, uniform=uniform, flags="SHAPE1", stride=80), rpl=2)
    assert is_v2_tail_outside(route(prog, uniform=uniform, flags="SHAPE1", stride=128), rpl=1, prefetch=0)


def test_all_general_beyond_stride_80_without_v2(prog):
    assert is_v2_tail_outside(route(prog, stride=80), rpl=1)
    assert is_v2_tail_outside(route(prog, stride=88), rpl=1, prefetch=0)
    assert three(route(prog, stride=80, v2_ok=0)) == ("pair", 20, 0, 1, "rescue")
    assert three(route(prog, stride=88, v2_ok=0)) == ("pair", 20, 1, 0, "list")
    assert three(route(prog, stride=40, v2_ok=0)) == ("pair", 10, 0, 1, "rescue")
    assert three(route(prog, stride=48, v2_ok=0)) == ("pair", 20, 0, 1, "rescue")


def test_v2_entries_hold_30_bit_read_indices(prog):
    assert is_fused_v2(route(prog, n_reads=2**30 - 1))
    assert three(route(prog, n_reads=2**30)) == ("pair", 10, 0, 1, "rescue")


def test_fuse_limit(prog):
    assert is_fused_v2(route(prog, trans1=64 * KB))
    assert is_v2_tail_outside(route(prog, trans1=64 * KB + 32))
    assert is_fused_v2(route(prog, trans1=64 * KB + 32, trans0=0, orientation="reverse", fuse_limit=64 * KB + 32))
    assert is_v2_tail_outside(route(prog, trans1=54 * KB + 32, fuse_limit=54 * KB))


def test_v2_lds_fit(prog):
    assert is_v2_tail_outside(route(prog, scan1=LDS_CU))      # the scan fits, no ring beside it
    assert three(route(prog, scan1=LDS_CU + 1)) == ("pair", 10, 0, 1, "rescue")
    assert is_fused_v2(route(prog, finish1=64 * KB))
    assert three(route(prog, finish1=64 * KB + 1)) == ("pair", 10, 0, 1, "rescue")
    # the other frame's tables do not matter to a one-frame call
    assert is_fused_v2(route(prog, scan0=LDS_CU + 1, finish0=64 * KB + 1))
    assert route(prog, scan0=LDS_CU + 1, orientation="forward")["form"] == "three"


@pytest.mark.parametrize("flag,expect", [
    ("V1_KERNELS", ("pair", 10, 0, 1, "rescue")),
    ("FORCE_SLOW_READER", ("pair", 10, 1, 0, "list")),
    ("ONE_BASE_SCAN", ("one_base", 10, 0, 0, "list")),
    ("LIST_RESCUE", ("pair", 10, 0, 0, "list")),
    ("PROFILE_LIST_SCAN_ONLY", ("pair", 10, 0, 1, "rescue")),
])
def test_each_flag_that_keeps_the_three_launch_form(prog, flag, expect):
    assert three(route(prog, flags=flag)) == expect


@pytest.mark.parametrize("flag", ["V2_NO_FUSE", "V2_SIDE_STREAMS", "V2_LEAN_SERIAL", "V2_NO_LEAN_RESCUE", "PROFILE_SCAN_ONLY",
                                  "PROFILE_RESCUE_HITS_ONLY", "PROFILE_NO_FINISH", "PROFILE_NO_EVENTS", "PROFILE_NO_TAIL"])
def test_each_flag_that_keeps_the_tail_out_of_the_scan(prog, flag):
    assert is_v2_tail_outside(route(prog, flags=flag))


def test_tail_stream_only_keeps_the_ring(prog):
    assert is_fused_v2(route(prog, flags="PROFILE_TAIL_STREAM_ONLY"))


def both(r):
    return (r["form"], r["last_form"], r["needs_tail_list"], r["passes"], r["frame0"], r["ring0"], r["frame1"], r["ring1"])


def test_both_is_two_passes_reverse_first(prog):
    assert both(route(prog, orientation="both")) == ("v2_both", 2, 0, 2, 1, 16, 0, 16)
    # one frame fuses, the other does not (config 2 under a fuse limit of 54 KB): the call needs the tail list
    assert both(route(prog, orientation="both", trans0=56608, trans1=53152, fuse_limit=54 * KB)) == ("v2_both", 2, 1, 2, 1, 16, 0, 0)
    assert both(route(prog, orientation="both", trans0=53152, trans1=56608, fuse_limit=54 * KB)) == ("v2_both", 2, 1, 2, 1, 0, 0, 16)
    assert both(route(prog, orientation="both", flags="V2_NO_FUSE")) == ("v2_both", 2, 1, 2, 1, 0, 0, 0)


@pytest.mark.parametrize("facts", [{"scan0": LDS_CU + 1}, {"scan1": LDS_CU + 1}, {"finish0": 64 * KB + 1}, {"finish1": 64 * KB + 1},
                                   {"flags": "PROFILE_NO_FINISH"}, {"flags": "PROFILE_TAIL_STREAM_ONLY"}, {"flags": "PROFILE_SCAN_ONLY"},
                                   {"flags": "V1_KERNELS"}, {"v2_ok": 0}, {"n_reads": 2**30}])
def test_both_without_v2_goes_through_the_list_kernel(prog, facts):
    assert three(route(prog, orientation="both", **facts)) == ("pair", 10, 1, 0, "list")


def test_both_fits_at_the_limits(prog):
    assert route(prog, orientation="both", scan0=LDS_CU, scan1=LDS_CU, finish0=64 * KB, finish1=64 * KB)["form"] == "v2_both"


def test_ring_sizes(prog):
    # room for four batches and not for eight: 163 840 - (scan + 8 192 + 2 048) = 15 360 = 4 * 3 840 at scan = 138 240
    assert is_v2_tail_outside(route(prog, scan1=138240, ring_min=8))
    assert is_fused_v2(route(prog, scan1=138240, ring_min=4), ring=4)
    assert is_v2_tail_outside(route(prog, scan1=138241, ring_min=4))
    # room for eight (30 720) and not for sixteen (61 440)
    assert is_fused_v2(route(prog, scan1=138240 - 15360), ring=8)
    assert is_fused_v2(route(prog, scan1=138240 - 15360 + 1, ring_min=4), ring=4)
    assert is_fused_v2(route(prog, scan1=163840 - 10240 - 61440), ring=16)
    assert is_fused_v2(route(prog, scan1=163840 - 10240 - 61440 + 1), ring=8)
    # the forced rings (DCRX_DEBUG_RING_BATCHES)
    assert is_fused_v2(route(prog, ring_max=4, ring_min=4), ring=4)
    assert is_fused_v2(route(prog, ring_max=8, ring_min=4), ring=8)
    # side tables and buckets count: 40 000 bytes more leave 163 840 - 108 096 = 55 744, room for eight batches (30 720), not sixteen
    assert is_fused_v2(route(prog, side=8192 + 40000), ring=8)
    assert is_fused_v2(route(prog, bucket1=2048 + 40000, bucket0=0), ring=8)


@pytest.mark.parametrize("facts,expect", [
    ({}, ("pair", 10, 0, 1, "rescue")),
    ({"pair_rescue": 0}, ("pair", 10, 0, 0, "list")),
    ({"flags": "V1_KERNELS+LIST_RESCUE"}, ("pair", 10, 0, 0, "list")),
    ({"lds16_bytes": LDS_CU - 36928}, ("pair", 10, 0, 1, "rescue")),
    ({"lds16_bytes": LDS_CU - 36928 + 1}, ("pair", 10, 0, 0, "list")),
    ({"lds16_bytes": LDS_CU - 4096, "rescue_lds_extra": 4096}, ("pair", 10, 0, 1, "rescue")),
    ({"table16_in_lds": 0}, ("one_base", 10, 0, 0, "list")),
    ({"table_in_lds": 0}, ("one_base", 10, 0, 0, "list")),
    ({"flags": "V1_KERNELS+ONE_BASE_SCAN"}, ("one_base", 10, 0, 0, "list")),
    ({"flags": "V1_KERNELS+FORCE_SLOW_READER"}, ("pair", 10, 1, 0, "list")),
    ({"orientation": "both"}, ("pair", 10, 1, 0, "list")),
    ({"stride": 88}, ("pair", 20, 1, 0, "list")),
])
def test_rescue_kernel_conditions_one_at_a_time(prog, facts, expect):
    facts = dict(facts)
    facts["flags"] = facts.get("flags", "V1_KERNELS")
    assert three(route(prog, **facts)) == expect
