"""Helpers of the error-merge tests (test_nbc_merge.py on CPU, test_gpu_nbc_merge.py on the GPU): the contract of
`--merge-errors` written directly in Python (expected_merge: strings, a dict of buckets, all pairs), noisy clonal reads that
remember where they were substituted, hand-made counted tables, and the brute force as a stand-in for nat.merge_dcrs."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from tests import chains_util as chu
from tests import nbc_count_util as nu
from tests import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))
ANCHOR = 32
MAX_JUNCTION = 128
ACGT = set("ACGT")


def inserts(counted):
    text, off = counted["ins_text"], [int(x) for x in counted["ins_off"]]
    return [text[off[k]:off[k + 1]].decode("latin-1") for k in range(len(off) - 1)]


def junction_of(ts, v, j, vdel, jdel, ins):
    """(junction, in reach) of one entry: the contract's two definitions, on strings."""
    Vr, Jr = ts.v_regions[v].upper(), ts.j_regions[j].upper()
    aV, aJ = min(ANCHOR, len(Vr)), min(ANCHOR, len(Jr))
    if vdel > aV or jdel > aJ:
        return None, False
    if not (set(ins) <= ACGT and set(Vr[len(Vr) - aV:]) <= ACGT and set(Jr[:aJ]) <= ACGT):
        return None, False
    junction = Vr[len(Vr) - aV:len(Vr) - vdel] + ins + Jr[jdel:aJ]
    if len(junction) > MAX_JUNCTION:
        return None, False
    return junction, True


def expected_merge(counted, ts, D, R):
    """The contract, directly: (merged table, statistics, root_of) of a counted table (entry k = rank k)."""
    n = len(counted["v"])
    v, j, vdel, jdel = (counted[f].tolist() for f in ("v", "j", "vdel", "jdel"))
    count, first = [int(x) for x in counted["count"]], [int(x) for x in counted["first"]]
    ins = inserts(counted)
    reach = [False] * n
    buckets = collections.defaultdict(list)
    junc = {}
    for k in range(n):
        s, ok = junction_of(ts, v[k], j[k], vdel[k], jdel[k], ins[k])
        reach[k] = ok
        if ok:
            junc[k] = s
            buckets[(v[k], j[k], len(s))].append(k)
    parent = list(range(n))
    for (_, _, length), members in buckets.items():          # members: ascending rank
        if len(members) < 2:
            continue
        M = np.frombuffer("".join(junc[k] for k in members).encode(), np.uint8).reshape(len(members), length)
        cnt = np.array([count[k] for k in members], dtype=np.uint64)
        for i in range(1, len(members)):
            ok = np.nonzero(cnt[:i] // np.uint64(R) >= cnt[i])[0]          # rank_p < rank_c by position
            if len(ok) == 0:
                continue
            ham = (M[ok] != M[i]).sum(axis=1)
            hit = np.nonzero(ham <= D)[0]
            if len(hit):
                parent[members[i]] = members[int(ok[hit[0]])]
    root_of, depth = list(range(n)), [0] * n
    for k in range(n):          # a parent's rank is smaller: its root is known
        if parent[k] != k:
            root_of[k], depth[k] = root_of[parent[k]], depth[parent[k]] + 1
    tot, fst = list(count), list(first)
    for k in range(n):
        if root_of[k] != k:
            tot[root_of[k]] += count[k]
            fst[root_of[k]] = min(fst[root_of[k]], first[k])
    roots = sorted((k for k in range(n) if root_of[k] == k), key=lambda k: (-tot[k], fst[k], k))
    merged = [k for k in range(n) if root_of[k] != k]
    stats = {"entries_in": n, "roots_out": len(roots), "out_of_reach": n - sum(reach), "merged": len(merged),
             "reads_moved": sum(count[k] for k in merged), "longest_chain": max(depth, default=0)}
    out = table([(v[k], j[k], vdel[k], jdel[k], ins[k], tot[k], fst[k]) for k in roots])
    return out, stats, np.array(root_of, np.uint32)


def table(entries):
    """A counted table (the dict DcrCounts.read() gives) of (v, j, vdel, jdel, insert, count, first) entries, as given."""
    ins = [e[4].encode("latin-1") for e in entries]
    off = np.zeros(len(entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in ins], dtype=np.uint64)
    return {"v": np.array([e[0] for e in entries], np.uint16), "j": np.array([e[1] for e in entries], np.uint16),
            "vdel": np.array([e[2] for e in entries], np.uint8), "jdel": np.array([e[3] for e in entries], np.uint8),
            "count": np.array([e[5] for e in entries], np.uint64), "first": np.array([e[6] for e in entries], np.uint64),
            "ins_off": off, "ins_text": b"".join(ins)}


def ranked(entries):
    """table() of entries put in rank order (count descending, ties by first ordinal)."""
    return table(sorted(entries, key=lambda e: (-e[5], e[6])))


def same_table(a, b):
    for f in ("v", "j", "vdel", "jdel", "count", "first", "ins_off"):
        assert np.array_equal(np.asarray(a[f]).astype(np.uint64), np.asarray(b[f]).astype(np.uint64)), f
    assert a["ins_text"] == b["ins_text"]


def counted_from_keys(keys):
    """The counted table of per-read DCR keys in file order (nu.read_dcrs): Counter.most_common() with first ordinals."""
    oc = nu.OracleCounts()
    for k, key in enumerate(keys):
        if key is not None:
            f = key.split(", ")
            oc.add((int(f[0]), int(f[1]), int(f[2]), int(f[3]), f[4]), k)
    return oc.read()


def noisy_clonal_reads(ts, n_reads, seed, n_pool=400, zipf=1.2, sub_rate=0.005, orientation="reverse"):
    """n_reads reads drawn with Zipf weights from a pool of n_pool pristine synthetic reads of `ts` (no substitutions, no
    N), every copy then given its own substitutions at sub_rate per base.  Returns (reads, clone: the pool index of every
    read, places: per read the array of substituted positions, pool: the pristine reads)."""
    rng = np.random.default_rng(seed)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    b = nat.synth_reads_host(t, nat.synth_cfg(seed=seed, p_rearranged=0.9, sub_rate=0.0, n_rate=0.0), 0, n_pool)
    pool = nat.unpack_reads(b)
    if orientation in ("forward", "both"):
        flip = rng.random(n_pool) < (1.0 if orientation == "forward" else 0.5)
        pool = [dec.revcomp(r) if f else r for r, f in zip(pool, flip)]
    w = 1.0 / np.arange(1, n_pool + 1) ** zipf
    clone = rng.choice(n_pool, size=n_reads, p=w / w.sum())
    L = len(pool[0])
    assert all(len(r) == L for r in pool)
    P = np.frombuffer("".join(pool).encode(), np.uint8).reshape(n_pool, L)
    code = np.zeros(256, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    reads, places = [], []
    for lo in range(0, n_reads, 100_000):          # (in parts: a mask of doubles over every base is large)
        part = P[clone[lo:lo + 100_000]].copy()
        hit = rng.random(part.shape) < sub_rate
        shift = rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)          # another base, never the same
        part[hit] = np.frombuffer(b"ACGT", np.uint8)[(code[part[hit]] + shift) & 3]
        rows, cols = np.nonzero(hit)
        places += np.split(cols, np.searchsorted(rows, np.arange(1, len(part))))
        text = part.tobytes().decode()
        reads += [text[k * L:(k + 1) * L] for k in range(len(part))]
    return reads, clone, places, pool


def out_of_reach_share(counted, ts):
    n = len(counted["v"])
    ins = inserts(counted)
    out = sum(1 for k in range(n) if not junction_of(ts, int(counted["v"][k]), int(counted["j"][k]), int(counted["vdel"][k]),
                                                     int(counted["jdel"][k]), ins[k])[1])
    return out / max(1, n)


class MergeTables(chu.OracleTables):
    """The CPU tests' tables stand-in that also remembers its regions (what the brute force needs of a tag set)."""

    def __init__(self, v_tags, v_jumps, v_regions, j_tags, j_jumps, j_regions, v_half_split, j_half_split):
        super().__init__(v_tags, v_jumps, v_regions, j_tags, j_jumps, j_regions, v_half_split, j_half_split)
        self.v_regions, self.j_regions = list(v_regions), list(j_regions)


class BruteMerge:
    """Stands expected_merge in for nat.merge_dcrs (after nu.OracleCountDevice has stood the oracle in for the count)."""

    def __init__(self, monkeypatch):
        self.calls = []          # (entries, distance, ratio)
        monkeypatch.setattr(nat, "Tables", MergeTables)
        monkeypatch.setattr(nat, "merge_dcrs", self.merge_dcrs)

    def merge_dcrs(self, tables, counted, distance=1, ratio=10):
        self.calls.append((len(counted["v"]), distance, ratio))
        return expected_merge(counted, tables, distance, ratio)


def host_merge_lib():
    d = os.path.join(HERE, "host_merge")
    subprocess.check_call(["make", "-s", "-C", d])
    L = C.CDLL(os.path.join(d, "build", "libmerge_host.so"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.merge_host_win_words.restype = u32
    L.merge_host_words.restype = u32
    L.merge_host_window.restype = None
    L.merge_host_window.argtypes = [C.c_char_p, u32, C.c_int, vp]
    L.merge_host_encode.restype = C.c_int
    L.merge_host_encode.argtypes = [vp, vp, u32, u32, vp, u64, vp, vp]
    L.merge_host_distance.restype = u32
    L.merge_host_distance.argtypes = [vp, vp, u32]
    L.merge_host_key.restype = u64
    L.merge_host_key.argtypes = [u32, u32, u32]
    L.merge_host_parents.restype = None
    L.merge_host_parents.argtypes = [vp, u32, u64, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, vp]
    return L


def host_windows(L, ts):
    ww = L.merge_host_win_words()
    rows = np.zeros((len(ts.v_regions) + len(ts.j_regions), ww), np.uint32)
    for k, r in enumerate(ts.v_regions):
        L.merge_host_window(r.upper().encode(), len(r), 1, rows[k].ctypes.data)
    for k, r in enumerate(ts.j_regions):
        L.merge_host_window(r.upper().encode(), len(r), 0, rows[len(ts.v_regions) + k].ctypes.data)
    return rows


def host_parents(L, ts, counted, D, R):
    """(parent, reach) of the host build's parents step over a counted table."""
    rows = host_windows(L, ts)
    n = len(counted["v"])
    arrs = [np.ascontiguousarray(counted[f]) for f in ("v", "j", "vdel", "jdel", "count", "ins_off")]
    text = np.frombuffer(counted["ins_text"] + b"\0", np.uint8)
    parent, reach = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint8)
    L.merge_host_parents(rows.ctypes.data, len(ts.v_regions), n, *[a.ctypes.data for a in arrs], text.ctypes.data, D, R,
                         parent.ctypes.data, reach.ctypes.data)
    return parent[:n], reach[:n]


def roots_of(parent):
    root = np.arange(len(parent))
    for k in range(len(parent)):
        if parent[k] != k:
            root[k] = root[parent[k]]
    return root.astype(np.uint32)
