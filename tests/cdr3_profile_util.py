"""What the radius-profile tests share (include/dcrx.h "profile, weighted"): the contract as plain Python that shares no method
with the kernel — every query against every target of its class through tests/cdr3_wmatch_util.dist_memo (the gapped string
built literally for every p), the bin -(-d // step) —, the stand-in for the native call, the device entry on a case, and the host
build of the walk with the histogram sink (tests/host_cdr3profile)."""
import ctypes as C
import os

import numpy as np

from decombinator_amd import _native as nat

from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_cdr3profile")
HOST_LIB = os.path.join(HOST_DIR, "build", "libcdr3profile_host.so")
Case = mu.Case


# ---- the contract ----

def expected_profile(case: Case, cost, step: int, bins: int) -> np.ndarray:
    """What nat.cdr3_profile_weighted gives as "profile", from the contract: (m_q, bins) uint32, cell [i, b] the targets j of
    query i's class, both taking part, with ceil(dist(i, j) / step) == b.  Every pair of a class is summed, whatever its lengths."""
    assert 1 <= step <= 65535 and 1 <= bins <= 32 and step * (bins - 1) <= 65535
    out = np.zeros((len(case.q_strings), bins), dtype=np.uint32)
    t_ok = [wu.in_reach(t) for t in case.t_strings]
    for i, (qc, q) in enumerate(zip(case.q_classes, case.q_strings)):
        if not wu.in_reach(q):
            continue
        for j, (c, t) in enumerate(zip(case.t_classes, case.t_strings)):
            if c == qc and t_ok[j]:
                b = -(-wu.dist_memo(q, t, cost) // step)
                if b < bins:
                    out[i, b] += 1
    return out


def expected_profile_numpy(case: Case, cost, step: int, bins: int) -> np.ndarray:
    """expected_profile() for larger tables: the hits within the ladder's top and their distances from wu.expected_numpy (the same
    literal minimum over every p, in numpy), each counted in bin -(-d // step)."""
    want = wu.expected_numpy(case, cost, step * (bins - 1))
    out = np.zeros((len(case.q_strings), bins), dtype=np.uint32)
    owner = np.repeat(np.arange(len(case.q_strings)), np.diff(want["hit_off"].astype(np.int64)))
    np.add.at(out, (owner, -(-want["hit_dist"].astype(np.int64) // step)), 1)
    return out


def expected_stats(case: Case, profile) -> dict:
    length_ok = lambda s: 1 <= len(s) <= wu.MAX_LEN
    rows = np.asarray(profile, dtype=np.uint64).sum(axis=1)      # (m_q, bins)
    assert len(rows) == len(case.q_strings)
    out = {"queries": len(case.q_strings), "targets": len(case.t_strings),
           "queries_out_of_reach": sum(not length_ok(s) for s in case.q_strings),
           "queries_not_letters": sum(length_ok(s) and not wu.letters(s) for s in case.q_strings),
           "targets_out_of_reach": sum(not length_ok(s) for s in case.t_strings),
           "cells_sum": int(rows.sum()), "queries_nonzero": int((rows > 0).sum())}
    assert tuple(out) == nat.CDR3_PROFILE_STATS
    return out


def ladder_for(R: int, step: int):
    """(step, bins) of the ladder 0, step, .. that reaches R or the 32nd rung, whichever comes first."""
    return step, min(-(-R // step) + 1, nat.CDR3_PROFILE_MAX_BINS)


def brute_force_native(calls=None):
    """What stands in for nat.cdr3_profile_weighted: the contract, in the native function's shape (index: a mu.StubIndex)."""
    def cdr3_profile_weighted(index, classes, off, text, cost, step, bins):
        strings = cnu.node_strings(off, text)
        if calls is not None:
            calls.append((index, np.asarray(classes).tolist(), strings, cost, int(step), int(bins)))
        case = Case(index.classes, index.strings, classes, strings)
        profile = expected_profile(case, cost, int(step), int(bins))
        return {"profile": profile, "stats": expected_stats(case, profile)}
    return cdr3_profile_weighted


# ---- the two entries on a case (GPU) ----

def native_profile(case: Case, cost, step: int, bins: int, index=None) -> dict:
    """nat.cdr3_profile_weighted (the host entry) on a case."""
    t_args, (qc, off, text, _) = mu.native_args(case)
    own = index or nat.Cdr3Index(*t_args)
    try:
        return nat.cdr3_profile_weighted(own, qc, off, text, cost, step, bins)
    finally:
        if index is None:
            own.close()


class DeviceQueries:
    """A case's queries in device memory, for nat.cdr3_profile_weighted_device."""

    def __init__(self, case: Case):
        _, (qc, off, text, _) = mu.native_args(case)
        self.m, self.text_bytes = len(qc), len(text)
        self.d_cls = nat.DeviceBuffer.from_host(np.ascontiguousarray(qc if self.m else np.zeros(1, np.uint32)))
        self.d_off = nat.DeviceBuffer.from_host(np.ascontiguousarray(off))
        self.d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))

    def args(self):
        return self.m, self.d_cls, self.d_off, self.d_text, self.text_bytes


def device_profile(case: Case, cost, step: int, bins: int, index=None, stream=None) -> np.ndarray:
    """nat.cdr3_profile_weighted_device on a case: the profile buffer prefilled with 0xA5, a work space of exactly work_bytes."""
    own = index or nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        q = DeviceQueries(case)
        cells = q.m * bins
        d_profile = nat.DeviceBuffer.from_host(np.full(max(cells, 1), 0xA5A5A5A5, np.uint32))
        work = nat.cdr3_profile_weighted_work_bytes(q.m, q.text_bytes, bins)
        assert work > 0
        d_work = nat.DeviceBuffer(work)
        nat.cdr3_profile_weighted_device(own, *q.args(), cost, step, bins, d_profile, d_work, work, stream)
        nat.synchronize()
        return d_profile.to_host(np.uint32, max(cells, 1))[:cells].reshape(q.m, bins)
    finally:
        if index is None:
            own.close()


# ---- bin_of and the walk with the histogram sink on the host (tests/host_cdr3profile) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", HOST_DIR])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        _host.cdr3profile_host_bins.restype = None
        _host.cdr3profile_host_bins.argtypes = [u32, u32, vp]
        _host.cdr3profile_host_refuses.restype = C.c_int
        _host.cdr3profile_host_refuses.argtypes = [u32, u32]
        _host.cdr3profile_host_profile.restype = C.c_int
        _host.cdr3profile_host_profile.argtypes = [u64, vp, vp, vp] * 2 + [vp, u32, u32, u32, u32, u32, vp]
    return _host


def host_bins(step: int, n: int = 65536) -> np.ndarray:
    """bin_of(d, step) of the shared header for every d in 0 .. n - 1."""
    out = np.zeros(n, np.uint32)
    host_lib().cdr3profile_host_bins(n, step, out.ctypes.data)
    return out


def host_profile(case: Case, cost, step: int, bins: int) -> np.ndarray:
    """The host walk with the histogram sink: (m_q, bins)."""
    (tc, t_off, t_text), (qc, q_off, q_text, _) = mu.native_args(case)
    tt, qt = (np.frombuffer(x + b"\0", np.uint8) for x in (t_text, q_text))
    sub = np.ascontiguousarray(cost.sub, dtype=np.uint8)
    m_q = len(qc)
    out = np.zeros(max(m_q * bins, 1), np.uint32)
    rc = host_lib().cdr3profile_host_profile(len(tc), tc.ctypes.data, t_off.ctypes.data, tt.ctypes.data, m_q, qc.ctypes.data, q_off.ctypes.data,
                                             qt.ctypes.data, sub.ctypes.data, cost.gap, cost.ntrim, cost.ctrim, step, bins, out.ctypes.data)
    assert rc == 0
    return out[:m_q * bins].reshape(m_q, bins)
