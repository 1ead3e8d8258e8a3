"""The radius profile (include/dcrx.h "profile, weighted") without a GPU: bin_of of the shared header against Python for every
distance, the host walk with the histogram sink against the contract (tests/cdr3_profile_util.py) on lists of
tests/cdr3_wmatch_util.py, the stand-alone program plain and under sanitizers, the exports, and every refusal of the two entries,
which is decided on the host before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from decombinator_amd import _native as nat
from tests import cdr3_profile_util as pu
from tests import cdr3_wmatch_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


# ---- bin_of ----

@pytest.mark.parametrize("step", [1, 2, 3, 5, 7, 12, 255, 256, 4095, 65535])
def test_bin_of_is_the_ceiling_for_every_distance(step):
    want = np.array([-(-d // step) for d in range(65536)], dtype=np.uint32)
    assert want[0] == 0 and want[1] == 1 and want[step] == 1 and (step == 65535 or want[step + 1] == 2)
    assert np.array_equal(pu.host_bins(step), want)


def test_the_ladders_the_shared_header_refuses():
    refuses = pu.host_lib().cdr3profile_host_refuses
    assert [refuses(*x) for x in ((0, 1), (1, 0), (1, 33), (65536, 1), (65535, 3), (2115, 32))] == [1] * 6
    assert [refuses(*x) for x in ((1, 1), (1, 32), (65535, 1), (65535, 2), (2114, 32), (2, 25))] == [0] * 6


# ---- the host walk with the histogram sink ----

def _lists():
    out = {}
    for make in (wu.single_pairs, wu.gap_positions, wu.large_sums, wu.trims):
        out.update(make())
    return out


def _ladders(R):
    """The ladders a list is walked under: step 1 up to R or the 32nd rung, step 3, tcrdist3's (2, 25), and R in one step."""
    out = {pu.ladder_for(R, 1), pu.ladder_for(R, 3), (2, 25)}
    if R > 0:
        out.add((R, 2))
    return sorted(out)


@pytest.mark.parametrize("name", sorted(_lists()))
def test_host_walk_against_the_contract(name):
    case, cost, R = _lists()[name]
    for step, bins in _ladders(R):
        want = pu.expected_profile(case, cost, step, bins)
        if R % step == 0 and R // step < bins:      # the premise: the prefix sums up to R's rung are the list's own degrees
            upto = np.asarray(want, dtype=np.int64)[:, :R // step + 1].sum(axis=1)
            assert upto.tolist() == wu.expected(case, cost, R)["degree"].tolist()
        assert np.array_equal(pu.host_profile(case, cost, step, bins), want), (name, step, bins)


def test_host_walk_bin_boundaries():
    near, cost, _ = wu.single_pairs()["conservative_at_cost"]      # one pair at distance 3
    for step, b in ((1, 3), (2, 2), (3, 1), (4, 1)):
        want = pu.expected_profile(near, cost, step, 4)
        assert want.tolist() == [[int(k == b) for k in range(4)]]
        assert np.array_equal(pu.host_profile(near, cost, step, 4), want)
    big, cost, _ = wu.large_sums()["sums_past_2_12"]               # pairs at exactly 8 160
    for step, bins in ((272, 31), (8159, 2), (65535, 2), (1, 1)):
        want = pu.expected_profile(big, cost, step, bins)
        assert np.array_equal(pu.host_profile(big, cost, step, bins), want)
    assert pu.expected_profile(big, cost, 272, 31)[0].tolist() == [0] * 30 + [2]      # both targets at 8 160 = 30 * 272: the last bin
    assert pu.expected_profile(big, cost, 8159, 2)[0].tolist() == [0, 0]              # 8 160 = R + 1: in no bin


def test_the_stand_alone_program_plain_and_under_sanitizers():
    """bin_of, the ladders and the host walk in a program of their own (its own main), never loaded into Python."""
    pu.host_lib()
    here = os.path.join(ROOT, "tests", "host_cdr3profile")
    plain = subprocess.run([os.path.join(here, "build", "cdr3profile_main")], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "ok", plain.stdout[-2000:]
    san = subprocess.run(["make", "-s", "-C", here, "asan"], capture_output=True, text=True)
    assert san.returncode == 0 and san.stdout.splitlines()[-1] == "ok", (san.stdout[-2000:], san.stderr[-2000:])


# ---- exports and ABI ----

def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    for name in ("dcrx_cdr3_profile_weighted_work_bytes", "dcrx_cdr3_profile_weighted_device", "dcrx_cdr3_profile_weighted"):
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(nat.lib(), name)
    assert "profile, weighted" in hdr
    fields = re.search(r"typedef struct dcrx_cdr3_profile_stats \{(.*?)\}", hdr, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == nat.CDR3_PROFILE_STATS
    assert C.sizeof(nat.Cdr3ProfileStatsC) == 8 * len(nat.CDR3_PROFILE_STATS)
    assert callable(nat.cdr3_profile_weighted) and callable(nat.cdr3_profile_weighted_device) and nat.CDR3_PROFILE_MAX_BINS == 32


def test_work_bytes_are_answered_on_the_host():
    need = nat.cdr3_profile_weighted_work_bytes(1000, 0, 25)
    assert need >= 1000 * (2 * 8 + 2 * 4 + 32) and need % 256 == 0      # two key and two rank arrays and the packed strings, at least
    assert nat.cdr3_profile_weighted_work_bytes(1000, 0, 1) == nat.cdr3_profile_weighted_work_bytes(1000, 0, 32) == need
    assert nat.cdr3_profile_weighted_work_bytes(1, 5, 25) > 0 and nat.cdr3_profile_weighted_work_bytes(0, 0, 25) > 0
    assert nat.cdr3_profile_weighted_work_bytes(1000, 0, 0) == 0 and nat.cdr3_profile_weighted_work_bytes(1000, 0, 33) == 0
    assert nat.cdr3_profile_weighted_work_bytes(1 << 30, 0, 25) == 0


# ---- the refusals of both entries: on the host, before any device call (an index of no targets touches no device) ----

def _empty_index():
    return nat.Cdr3Index(np.zeros(0, np.uint32), np.zeros(1, np.uint64), b"")


def _bad_settings():
    ok = nat.Cdr3Cost.default()
    asym, diag = ok.sub.copy(), ok.sub.copy()
    asym[1, 3] = 5
    diag[26, 26] = 1
    return [(nat.Cdr3Cost(asym), 2, 25, "symmetric"), (nat.Cdr3Cost(diag), 2, 25, "diagonal"), (nat.Cdr3Cost.default(gap=0), 2, 25, "gap"),
            (nat.Cdr3Cost.default(gap=256), 2, 25, "gap"), (nat.Cdr3Cost.default(ntrim=17), 2, 25, "trim"),
            (nat.Cdr3Cost.default(ctrim=17), 2, 25, "trim"), (None, 2, 25, "null cost"),
            (ok, 0, 25, "step"), (ok, 65536, 1, "step"), (ok, 2, 0, "bins"), (ok, 2, 33, "bins"), (ok, 65535, 3, "above 65535"),
            (ok, 2115, 32, "above 65535")]


class _Fake:
    """Something with a .ptr: an address the entry must refuse before it looks behind it."""

    def __init__(self, ptr):
        self.ptr = ptr


def test_both_entries_refuse_what_the_contract_refuses():
    index = _empty_index()
    cls, off, text = np.zeros(1, np.uint32), np.array([0, 5], np.uint64), b"CASSF"
    try:
        for cost, step, bins, msg in _bad_settings():
            with pytest.raises(nat.DcrxError, match=msg) as e:
                nat.cdr3_profile_weighted(index, cls, off, text, cost, step, bins)
            assert e.value.code == E_INVALID
            with pytest.raises(nat.DcrxError, match=msg) as e:
                nat.cdr3_profile_weighted_device(index, 0, None, None, None, 0, cost, step, bins, None, None, 0)
            assert e.value.code == E_INVALID
        ok, L = nat.Cdr3Cost.default(), nat.lib()
        c = ok.as_c()
        # a null profile with m_q > 0, on both entries; a null index; offsets that go backwards
        with pytest.raises(nat.DcrxError, match="null profile"):
            nat.cdr3_profile_weighted_device(index, 1, _Fake(256), _Fake(256), _Fake(256), 5, ok, 2, 25, None, _Fake(256), 1 << 20)
        o = np.array([0, 5], np.uint64)
        t = np.frombuffer(b"CASSF\0", np.uint8)
        assert L.dcrx_cdr3_profile_weighted(index.handle, 1, cls.ctypes.data, o.ctypes.data, t.ctypes.data, C.addressof(c), 2, 25, None, None) == E_INVALID
        assert b"null profile" in L.dcrx_last_error()
        assert L.dcrx_cdr3_profile_weighted(None, 0, None, None, None, C.addressof(c), 2, 25, None, None) == E_INVALID
        assert L.dcrx_cdr3_profile_weighted_device(None, 0, None, None, None, 0, C.addressof(c), 2, 25, None, None, 0, None) == E_INVALID
        back = np.array([5, 0], np.uint64)
        one = np.zeros(25, np.uint32)
        assert L.dcrx_cdr3_profile_weighted(index.handle, 1, cls.ctypes.data, back.ctypes.data, t.ctypes.data, C.addressof(c), 2, 25,
                                            one.ctypes.data, None) == E_INVALID and b"backwards" in L.dcrx_last_error()
        # the work space: misaligned, one byte short, null
        need = nat.cdr3_profile_weighted_work_bytes(1, 5, 25)
        with pytest.raises(nat.DcrxError, match="256-byte aligned"):
            nat.cdr3_profile_weighted_device(index, 1, _Fake(256), _Fake(256), _Fake(256), 5, ok, 2, 25, _Fake(256), _Fake(256 + 64), need)
        with pytest.raises(nat.DcrxError, match="smaller than dcrx_cdr3_profile_weighted_work_bytes"):
            nat.cdr3_profile_weighted_device(index, 1, _Fake(256), _Fake(256), _Fake(256), 5, ok, 2, 25, _Fake(256), _Fake(256), need - 1)
        with pytest.raises(nat.DcrxError, match="null argument"):
            nat.cdr3_profile_weighted_device(index, 1, _Fake(256), _Fake(256), _Fake(256), 5, ok, 2, 25, _Fake(256), None, need)
        with pytest.raises(ValueError):
            nat.cdr3_profile_weighted(index, cls, off, text, ok, -1, 25)
    finally:
        index.close()


def test_no_queries_and_no_targets_are_answered_on_the_host():
    index = _empty_index()
    try:
        ok = nat.Cdr3Cost.default()
        got = nat.cdr3_profile_weighted(index, np.zeros(0, np.uint32), np.zeros(1, np.uint64), b"", ok, 2, 25)
        assert got["profile"].shape == (0, 25) and got["stats"] == dict.fromkeys(nat.CDR3_PROFILE_STATS, 0)
        nat.cdr3_profile_weighted_device(index, 0, None, None, None, 0, ok, 2, 25, None, None, 0)      # nothing to write: no device call
        strings = [b"CASSF", b"", b"CAS*F", b"A" * 33, b"CASSW"]
        off = np.zeros(6, np.uint64)
        off[1:] = np.cumsum([len(s) for s in strings])
        got = nat.cdr3_profile_weighted(index, np.zeros(5, np.uint32), off, b"".join(strings), ok, 65535, 2)
        assert got["profile"].shape == (5, 2) and not got["profile"].any()      # (the buffer came uncleared: every cell was written)
        assert got["stats"] == {"queries": 5, "targets": 0, "queries_out_of_reach": 2, "queries_not_letters": 1, "targets_out_of_reach": 0,
                                "cells_sum": 0, "queries_nonzero": 0}
    finally:
        index.close()
