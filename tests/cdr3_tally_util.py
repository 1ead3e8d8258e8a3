"""What the tally tests share (include/dcrx.h "tally, weighted"): the contract as plain Python that shares no method with the kernel
— every query against every target of its class through tests/cdr3_wmatch_util.dist_memo (the gapped string built literally for
every p), a hit where the distance is at most the TARGET's own radius —, a numpy form for larger tables, the patterns of radii the
tests use, the stand-in for the native call, the two entries on a case, and the host build of the walk with the per-entry bound
and the tally sink (tests/host_cdr3tally)."""
import ctypes as C
import os

import numpy as np

from decombinator_amd import _native as nat

from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_cdr3tally")
HOST_LIB = os.path.join(HOST_DIR, "build", "libcdr3tally_host.so")
NO_RADIUS = 0xFFFFFFFF
MAX_RADIUS = 65535
Case = mu.Case


# ---- the contract ----

def _totals(case: Case, radii, pairs) -> dict:
    """The outputs and statistics from the hits (i, j)."""
    m_q, m_t = len(case.q_strings), len(case.t_strings)
    t_count, t_weight, q_degree = [0] * m_t, [0] * m_t, [0] * m_q
    for i, j in pairs:
        t_count[j] += 1
        t_weight[j] += case.weights[i]
        q_degree[i] += 1
    length_ok = lambda s: 1 <= len(s) <= wu.MAX_LEN
    stats = {"queries": m_q, "targets": m_t, "queries_out_of_reach": sum(not length_ok(s) for s in case.q_strings),
             "queries_not_letters": sum(length_ok(s) and not wu.letters(s) for s in case.q_strings),
             "targets_out_of_reach": sum(not length_ok(s) for s in case.t_strings),
             "targets_without_radius": sum(int(r) == NO_RADIUS for r in radii), "hits": sum(q_degree),
             "queries_hit": sum(d > 0 for d in q_degree), "queries_hit_weight": sum(w for w, d in zip(case.weights, q_degree) if d),
             "targets_hit": sum(c > 0 for c in t_count)}
    assert tuple(stats) == nat.CDR3_TALLY_STATS
    return {"t_count": np.array(t_count, dtype=np.uint32), "t_weight": np.array(t_weight, dtype=np.uint64),
            "q_degree": np.array(q_degree, dtype=np.uint32), "stats": stats}


def expected_tally(case: Case, cost, radii) -> dict:
    """What nat.cdr3_tally_weighted gives, from the contract: (i, j) is a hit when both take part, the classes agree, radii[j] is
    a radius (0 .. 65535) and dist(i, j) <= radii[j].  Every pair of a class is summed, whatever its lengths."""
    radii = [int(r) for r in radii]
    assert len(radii) == len(case.t_strings)
    t_ok = [wu.in_reach(t) and r <= MAX_RADIUS for t, r in zip(case.t_strings, radii)]
    pairs = []
    for i, (qc, q) in enumerate(zip(case.q_classes, case.q_strings)):
        if not wu.in_reach(q):
            continue
        for j, (c, t) in enumerate(zip(case.t_classes, case.t_strings)):
            if c == qc and t_ok[j] and wu.dist_memo(q, t, cost) <= radii[j]:
                pairs.append((i, j))
    return _totals(case, radii, pairs)


def expected_tally_numpy(case: Case, cost, radii) -> dict:
    """expected_tally() for larger tables: the hits within the largest radius and their distances from wu.expected_numpy (the same
    literal minimum over every p, in numpy), each kept where its distance is at most its target's own radius."""
    radii = np.array([int(r) for r in radii], dtype=np.int64)
    assert len(radii) == len(case.t_strings)
    has = radii <= MAX_RADIUS
    want = wu.expected_numpy(case, cost, int(radii[has].max()) if has.any() else 0)
    hit, dist = want["hit"].astype(np.int64), want["hit_dist"].astype(np.int64)
    owner = np.repeat(np.arange(len(case.q_strings), dtype=np.int64), np.diff(want["hit_off"].astype(np.int64)))
    keep = has[hit] & (dist <= radii[hit]) if len(hit) else np.zeros(0, bool)
    return _totals(case, radii.tolist(), zip(owner[keep].tolist(), hit[keep].tolist()))


PATTERNS = ("all_R", "graded", "every_third_none")


def radii_for(pattern: str, R: int, m_t: int) -> np.ndarray:
    """The radii per target by rank: all R; R * (j % 4) // 3 (0, a third, two thirds, R); every third target without one."""
    j = np.arange(m_t, dtype=np.int64)
    r = {"all_R": np.full(m_t, R, np.int64), "graded": R * (j % 4) // 3, "every_third_none": np.where(j % 3 == 2, NO_RADIUS, R)}[pattern]
    return r.astype(np.uint32)


def assert_same(got: dict, want: dict, what=""):
    for k in ("t_count", "t_weight", "q_degree"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    if "stats" in got:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def brute_force_native(calls=None, numpy_form=False):
    """What stands in for nat.cdr3_tally_weighted: the contract, in the native function's shape (index: a mu.StubIndex)."""
    def cdr3_tally_weighted(index, classes, off, text, weights, cost, radii):
        strings = cnu.node_strings(off, text)
        if calls is not None:
            calls.append((index, np.asarray(classes).tolist(), strings, np.asarray(weights).tolist(), cost, np.asarray(radii).tolist()))
        case = Case(index.classes, index.strings, classes, strings, weights)
        return (expected_tally_numpy if numpy_form else expected_tally)(case, cost, np.asarray(radii).tolist())
    return cdr3_tally_weighted


# ---- the two entries on a case (GPU) ----

def native_tally(case: Case, cost, radii, index=None) -> dict:
    """nat.cdr3_tally_weighted (the host entry) on a case."""
    t_args, q_args = mu.native_args(case)
    own = index or nat.Cdr3Index(*t_args)
    try:
        return nat.cdr3_tally_weighted(own, *q_args, cost, radii)
    finally:
        if index is None:
            own.close()


class DeviceQueries:
    """A case's queries (with their weights) in device memory, for nat.cdr3_tally_weighted_device."""

    def __init__(self, case: Case):
        _, (qc, off, text, w) = mu.native_args(case)
        self.m, self.text_bytes = len(qc), len(text)
        self.d_cls = nat.DeviceBuffer.from_host(np.ascontiguousarray(qc if self.m else np.zeros(1, np.uint32)))
        self.d_off = nat.DeviceBuffer.from_host(np.ascontiguousarray(off))
        self.d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
        self.d_weight = nat.DeviceBuffer.from_host(np.ascontiguousarray(w if self.m else np.zeros(1, np.uint64)))

    def args(self):
        return self.m, self.d_cls, self.d_off, self.d_text, self.text_bytes, self.d_weight


def device_radii(radii):
    r = np.ascontiguousarray(radii, dtype=np.uint32)
    return nat.DeviceBuffer.from_host(r if len(r) else np.zeros(1, np.uint32))


def device_tally(case: Case, cost, radii, index=None, stream=None) -> dict:
    """nat.cdr3_tally_weighted_device on a case: the outputs prefilled with 0xA5, a work space of exactly work_bytes."""
    own = index or nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        q, m_t = DeviceQueries(case), len(case.t_strings)
        d_tc = nat.DeviceBuffer.from_host(np.full(max(m_t, 1), 0xA5A5A5A5, np.uint32))
        d_tw = nat.DeviceBuffer.from_host(np.full(max(m_t, 1), 0xA5A5A5A5A5A5A5A5, np.uint64))
        d_deg = nat.DeviceBuffer.from_host(np.full(max(q.m, 1), 0xA5A5A5A5, np.uint32))
        work = nat.cdr3_tally_weighted_work_bytes(q.m, q.text_bytes, m_t)
        assert work > 0
        d_work, d_r = nat.DeviceBuffer(work), device_radii(radii)
        nat.cdr3_tally_weighted_device(own, *q.args(), cost, d_r, d_tc, d_tw, d_deg, d_work, work, stream)
        nat.synchronize()
        return {"t_count": d_tc.to_host(np.uint32, max(m_t, 1))[:m_t], "t_weight": d_tw.to_host(np.uint64, max(m_t, 1))[:m_t],
                "q_degree": d_deg.to_host(np.uint32, max(q.m, 1))[:q.m]}
    finally:
        if index is None:
            own.close()


# ---- the walk with the per-entry bound and the tally sink on the host (tests/host_cdr3tally) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", HOST_DIR])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        _host.cdr3tally_host_refuses.restype = C.c_int
        _host.cdr3tally_host_refuses.argtypes = [vp, u64]
        _host.cdr3tally_host_tally.restype = u64
        _host.cdr3tally_host_tally.argtypes = [u64, vp, vp, vp] * 2 + [vp, vp, u32, u32, u32, vp, vp, vp, vp]
    return _host


def host_refuses(radii) -> bool:
    """Whether the host entry refuses these radii (refuse_radii of the shared header)."""
    r = np.ascontiguousarray(radii, dtype=np.uint32)
    return bool(host_lib().cdr3tally_host_refuses(r.ctypes.data if len(r) else None, len(r)))


def host_tally(case: Case, cost, radii) -> dict:
    """The host walk with the tally sink; "flushes": the (block, staged entry) pairs that reached the accumulators."""
    (tc, t_off, t_text), (qc, q_off, q_text, w) = mu.native_args(case)
    tt, qt = (np.frombuffer(x + b"\0", np.uint8) for x in (t_text, q_text))
    sub = np.ascontiguousarray(cost.sub, dtype=np.uint8)
    r = np.ascontiguousarray(radii, dtype=np.uint32)
    m_q, m_t = len(qc), len(tc)
    t_count, t_weight, q_degree = np.zeros(max(m_t, 1), np.uint32), np.zeros(max(m_t, 1), np.uint64), np.zeros(max(m_q, 1), np.uint32)
    flushes = host_lib().cdr3tally_host_tally(m_t, tc.ctypes.data, t_off.ctypes.data, tt.ctypes.data, m_q, qc.ctypes.data, q_off.ctypes.data,
                                              qt.ctypes.data, w.ctypes.data, sub.ctypes.data, cost.gap, cost.ntrim, cost.ctrim,
                                              r.ctypes.data if m_t else None, t_count.ctypes.data, t_weight.ctypes.data, q_degree.ctypes.data)
    return {"t_count": t_count[:m_t], "t_weight": t_weight[:m_t], "q_degree": q_degree[:m_q], "flushes": int(flushes)}
