"""Helpers of the error-merge tests (test_nbc_merge.py on CPU, test_gpu_nbc_merge.py on the GPU): the contract of
`--merge-errors` written directly in Python (expected_merge: strings, a dict of buckets, all pairs), noisy clonal reads that
remember where they were substituted, hand-made counted tables, the brute force as a stand-in for nat.merge_dcrs, and the
constructed lists that pin the kernel's walk (each builder asserts its own premise on the contract; no GPU, no library)."""
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


def expected_parents(counted, ts, D, R):
    """The contract's parents step, directly: (parent, reach) of a counted table (entry k = rank k)."""
    n = len(counted["v"])
    v, j, vdel, jdel = (counted[f].tolist() for f in ("v", "j", "vdel", "jdel"))
    count = [int(x) for x in counted["count"]]
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
    return parent, reach


def expected_merge(counted, ts, D, R):
    """The contract, directly: (merged table, statistics, root_of) of a counted table (entry k = rank k)."""
    n = len(counted["v"])
    v, j, vdel, jdel = (counted[f].tolist() for f in ("v", "j", "vdel", "jdel"))
    count, first = [int(x) for x in counted["count"]], [int(x) for x in counted["first"]]
    ins = inserts(counted)
    parent, reach = expected_parents(counted, ts, D, R)
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


def take(counted, n):
    """The first n entries of a counted table."""
    out = {f: counted[f][:n].copy() for f in ("v", "j", "vdel", "jdel", "count", "first")}
    out["ins_off"] = counted["ins_off"][:n + 1].copy()
    out["ins_text"] = counted["ins_text"][:int(counted["ins_off"][n])]
    return out


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


# ---- constructed lists: merge_parents_kernel's walk, the counts and the primitive's rules.  Every builder asserts its own
# premise on the contract above (expected_parents / expected_merge) before it returns, so a list that stopped being the edge
# it was written for fails without a GPU.  With vdel = jdel = ANCHOR and windows of ANCHOR clean bases the junction is the
# insert alone (bare). ----

BASES = "ACGT"
TILE = 256          # merge_parents_kernel stages this many sorted entries per step, and a block holds this many children


def sub(s, p, step=1):
    """s with the base at p replaced by another one."""
    return s[:p] + BASES[(BASES.index(s[p]) + step) % 4] + s[p + 1:]


def subs(s, places):
    for p in places:
        s = sub(s, p)
    return s


def pack(s):
    """A junction as the kernels hold it: eight dwords of 2-bit bases, A = 0, zero beyond the length."""
    w = [0] * (MAX_JUNCTION // 16)
    for p, c in enumerate(s):
        w[p // 16] |= BASES.index(c) << (2 * (p % 16))
    return w


def packed_distance(a, b):
    """Bases at which two packed junctions differ, over all MAX_JUNCTION places (what the walk sees without the lengths)."""
    return sum(((x ^ y) >> (2 * p)) & 3 != 0 for x, y in zip(pack(a), pack(b)) for p in range(16))


def full_anchors(ts):
    """Whether every window of the tag set is ANCHOR clean bases (then bare() entries have the insert for a junction)."""
    return all(len(r) >= ANCHOR and set(r.upper()[-ANCHOR:]) <= ACGT for r in ts.v_regions) and \
        all(len(r) >= ANCHOR and set(r.upper()[:ANCHOR]) <= ACGT for r in ts.j_regions)


def bare(v, j, ins, count, first):
    return (v, j, ANCHOR, ANCHOR, ins, count, first)


def random_bases(rng, length):
    return "".join(rng.choice(list(BASES), size=length)) if length else ""


def junctions(counted, ts):
    """Per entry its junction, None where it is out of reach."""
    ins = inserts(counted)
    return [junction_of(ts, int(counted["v"][k]), int(counted["j"][k]), int(counted["vdel"][k]), int(counted["jdel"][k]), ins[k])[0]
            for k in range(len(ins))]


def sorted_order(counted, ts):
    """The ranks in the order the device puts them: by (v, j, junction length), stable, entries out of reach behind all."""
    junc = junctions(counted, ts)
    return sorted(range(len(junc)), key=lambda k: (1, 0, 0, 0) if junc[k] is None else
                  (0, int(counted["v"][k]), int(counted["j"][k]), len(junc[k])))


def _fillers(rng, n, count_from=9000):
    """One bucket (v 0, j 0, 30 bases) of n entries that are far apart, in front of every other bucket in sorted order; their
    counts are larger than any count behind them, so a walk that wrongly starts among them is not stopped by the ratio."""
    return [bare(0, 0, random_bases(rng, 30), count_from + n - k, k) for k in range(n)]


DECOY_LENGTHS = (15, 16, 31, 63, 64, 127)
DECOY_FILLERS = (1, 255, 256, 257, 300)          # the decoy buckets start at this sorted position


def padding_decoys(ts, length, n_fill, with_children):
    """List 1a.  X of `length` bases (its last one not A) and X[:-1], X + "A", X + "AA": four neighbouring buckets of one (v, j)
    whose packed junctions are equal (or one base apart) although the lengths differ.  Without children every bucket is a far
    head and the decoy behind it, and nothing merges; with children every bucket is the decoy and one substitution of it, and
    every bucket has exactly one merge.  n_fill entries of another bucket stand in front.  Returns (table, merges)."""
    assert full_anchors(ts)
    rng = np.random.default_rng(1000 * length + n_fill)
    X = random_bases(rng, length - 1) + str(rng.choice(list("CGT")))
    group, counts = [X[:-1], X, X + "A", X + "AA"], [40, 1000, 30, 20]
    assert all(pack(s) == pack(X) for s in group[1:] if len(s) <= MAX_JUNCTION) and packed_distance(X, X[:-1]) == 1
    entries = _fillers(rng, n_fill)
    first = n_fill
    for s, c in zip(group, counts):
        if with_children:
            entries += [bare(1, 0, s, c, first), bare(1, 0, sub(s, 0), 1, first + 1)]
        else:
            entries += [bare(1, 0, random_bases(rng, len(s)), 5000, first), bare(1, 0, s, c, first + 1)]
        first += 2
    counted = ranked(entries)
    junc = junctions(counted, ts)
    order = sorted_order(counted, ts)
    in_reach = [len(s) for s in group if len(s) <= MAX_JUNCTION]
    # the decoy buckets stand next to each other, in length order, from sorted position n_fill on
    assert [len(junc[k]) for k in order[:n_fill]] == [30] * n_fill
    assert [len(junc[k]) for k in order[n_fill:n_fill + 2 * len(in_reach)]] == [x for x in in_reach for _ in range(2)]
    for D in (1, 2):
        _, stats, root = expected_merge(counted, ts, D, 1)
        assert stats["out_of_reach"] == 2 * (len(group) - len(in_reach))
        assert stats["merged"] == (len(in_reach) if with_children else 0)
        if with_children:          # every child's root is its own bucket's head
            where = {s: k for k, s in enumerate(junc) if s is not None}
            assert all(root[where[sub(s, 0)]] == where[s] for s in group if len(s) <= MAX_JUNCTION)
    return counted, (len(in_reach) if with_children else 0)


def gene_pair_decoys(ts, axis):
    """List 1b.  One insert under two V genes and one J gene (axis "v"), or two J genes and one V gene (axis "j"): identical
    junctions in two neighbouring buckets.  The first bucket is H and its child; the second is a far head G, H again, a
    substitution of H and G's child.  The children merge inside their buckets (at R = 1 the substitution of H joins the H of
    its own bucket); nothing crosses, and the second H stays a root."""
    assert full_anchors(ts)
    rng = np.random.default_rng(77 + (axis == "j"))
    H, G = random_bases(rng, 40), random_bases(rng, 40)
    (va, ja), (vb, jb) = ((3, 2), (4, 2)) if axis == "v" else ((3, 2), (3, 3))
    counted = ranked([bare(va, ja, H, 1000, 0), bare(va, ja, sub(H, 5), 2, 1), bare(vb, jb, G, 900, 2), bare(vb, jb, H, 5, 3),
                      bare(vb, jb, sub(H, 9), 3, 4), bare(vb, jb, sub(G, 7), 1, 5)])
    assert inserts(counted) == [H, G, H, sub(H, 9), sub(H, 5), sub(G, 7)]
    assert sorted_order(counted, ts) == [0, 4, 1, 2, 3, 5]          # the two buckets stand next to each other
    for D, R in ((1, 10), (2, 1)):
        _, stats, root = expected_merge(counted, ts, D, R)
        assert root.tolist() == [0, 1, 2, 3 if R == 10 else 2, 0, 1] and stats["out_of_reach"] == 0
    return counted


PREFIX_PLACES = ((0, 3), (7, 3), (8, 3), (255, 3), (256, 3), (0, 0), (255, 0), (299, 0))          # (offset, entries up to the child)


def prefix_end(ts, R, k, gap, eligible):
    """List 1c.  One bucket that starts at sorted position 0, so bucket offsets are tile offsets.  Offsets 0 .. k-1 are far
    heads above R * c; offset k is one substitution from the child and has exactly R * c reads (eligible) or R * c - 1 (not);
    `gap` entries of R * c - 1 follow, the first of them one substitution from the child as well, with a first ordinal below
    the parent's; then the child of c reads.  Returns (table, the child's rank, its parent's rank or the child's own)."""
    assert full_anchors(ts)
    rng = np.random.default_rng(31 * k + 7 * gap + R)
    c = 7
    need = R * c
    child = random_bases(rng, 40)
    parent, decoy = sub(child, 3), sub(child, 20)
    entries = [bare(1, 2, random_bases(rng, 40), need + (k - i), i) for i in range(k)]
    entries.append(bare(1, 2, parent, need if eligible else need - 1, 1000))
    entries += [bare(1, 2, decoy if g == 0 else random_bases(rng, 40), need - 1, 999 if g == 0 else 1000 + g) for g in range(gap)]
    entries.append(bare(1, 2, child, c, 2000))
    counted = ranked(entries)
    at = {s: i for i, s in enumerate(inserts(counted))}
    count = [int(x) for x in counted["count"]]
    assert sorted_order(counted, ts) == list(range(len(entries)))          # one bucket, in rank order
    want = at[parent] if eligible else at[child]
    for D in (1, 2):
        assert expected_parents(counted, ts, D, R)[0][at[child]] == want
    if eligible:
        assert at[parent] == k and count[k] == need and (k == 0 or count[k - 1] > need)
        if k == 0:
            assert count[0] == need          # the early-out's edge: the bucket's largest count is exactly the need
        if R > 1:          # the prefix is cut at offset k + 1 (or the child stands there)
            assert at[child] == k + 1 + gap and (gap == 0 or count[k + 1] == need - 1)
    else:
        assert all(x != need for x in count[:at[child]]) and (k > 0 or R == 1 or count[0] == need - 1)
    if gap:
        # the decoy asks for a place in front of the parent (a smaller first ordinal); the rank order puts it behind
        assert at[decoy] > at[parent] or not eligible
        assert R == 1 or at[decoy] < at[child]
    return counted, at[child], want


BALL_PLACES = (0, 15, 16, 31, 32, 39)


def equal_counts_ball(ts, n=600):
    """List 1d.  One bucket of n entries of 5 reads each: strings that differ from one seed of 40 bases in at most three of six
    places (at the word edges), first ordinals a permutation.  With R = 1 every entry in front is eligible by count, so the
    parent is the smallest rank within distance, later candidates lose, and entries behind the child never count."""
    import itertools
    assert full_anchors(ts)
    rng = np.random.default_rng(1234)
    seed = random_bases(rng, 40)
    ball = sorted({subs_steps(seed, BALL_PLACES, steps) for steps in itertools.product(range(4), repeat=len(BALL_PLACES))
                   if sum(1 for x in steps if x) <= 3})
    assert len(ball) == 694 and n <= len(ball)
    picks = [ball[i] for i in rng.permutation(len(ball))[:n]]
    firsts = rng.permutation(n).tolist()
    counted = ranked([bare(1, 2, s, 5, f) for s, f in zip(picks, firsts)])
    M = np.frombuffer("".join(inserts(counted)).encode(), np.uint8).reshape(n, 40)
    ham = (M[:, None, :] != M[None, :, :]).sum(axis=2)
    for D in (1, 2):
        parent = expected_parents(counted, ts, D, 1)[0]
        near = ham <= D
        np.fill_diagonal(near, False)
        front = [np.nonzero(near[i, :i])[0] for i in range(n)]
        assert all(parent[i] == (int(front[i][0]) if len(front[i]) else i) for i in range(n))
        assert sum(1 for f in front if len(f) >= 2) >= n // 4          # a later candidate that must lose
        assert sum(1 for i in range(n) if near[i, i + 1:].any()) >= n // 4          # an entry behind that never is a parent
    return counted


def subs_steps(s, places, steps):
    for p, step in zip(places, steps):
        if step:
            s = sub(s, p, step)
    return s


CHAIN_LINKS = 384


def deep_chain(ts, n_out=0):
    """List 1e.  "A" * 128, then one place per entry turned A -> C from left to right, then C -> G, then G -> T: 385 entries of
    7 reads in rank order (by first ordinal), each one substitution from the one before and two from the one before that.
    n_out entries out of reach (an N in the insert) stand between them in rank order."""
    assert full_anchors(ts)
    s, chain = ["A"] * MAX_JUNCTION, ["A" * MAX_JUNCTION]
    for b in "CGT":
        for p in range(MAX_JUNCTION):
            s[p] = b
            chain.append("".join(s))
    assert len(chain) == CHAIN_LINKS + 1
    entries = []
    for i, x in enumerate(chain):
        entries.append(bare(1, 2, x, 7, len(entries)))
        if (i * n_out) // len(chain) < ((i + 1) * n_out) // len(chain):
            entries.append(bare(1, 2, "ACGTN", 7, len(entries)))
    counted = table(entries)
    assert len(entries) == len(chain) + n_out
    for D in (1, 2):
        _, stats, root = expected_merge(counted, ts, D, 1)
        assert stats == {"entries_in": len(entries), "roots_out": 1 + n_out, "out_of_reach": n_out, "merged": CHAIN_LINKS,
                         "reads_moved": 7 * CHAIN_LINKS, "longest_chain": CHAIN_LINKS // D}
    return counted


EDGE_PLACES = ((0,), (15,), (16,), (63,), (64,), (127,), (63, 64), (0, 127), (0, 1, 64), (62, 63, 64))


def lengths_and_word_edges(ts):
    """List 1f.  One (v, j) with junctions of 0, 1, 16, 17, 64, 65, 128 and 129 bases.  The buckets of 65 and 128 hold a base
    and children substituted at EDGE_PLACES (a place beyond the end stands for the last one): the first and last base of a
    dword, both sides of the half split at base 63/64, alone, in pairs and in threes.  The 17- and 65-base heads are the 16-
    and 64-base heads with an A behind them.  With R = 10 and children of 1 .. 9 reads only a head can be a parent.  Returns
    (table, {rank of a child: (rank of its head, substitutions)})."""
    assert full_anchors(ts)
    rng = np.random.default_rng(65)
    b16, b64, b128, b129 = (random_bases(rng, n) for n in (16, 64, 128, 129))
    entries, kids = [], []

    def bucket(head, count, places):
        entries.append(bare(2, 1, head, count, len(entries)))
        seen = set()
        for pl in places:
            pl = tuple(sorted({min(p, len(head) - 1) for p in pl}))
            if pl in seen:
                continue
            seen.add(pl)
            entries.append(bare(2, 1, subs(head, pl), 1 + len(kids) % 9, len(entries)))
            kids.append((subs(head, pl), head, len(pl)))
    entries += [bare(2, 1, "", 50, 0), bare(2, 1, "", 4, 1)]
    bucket("C", 1000, [(0,)])
    bucket(b16, 1000, [(0,), (15,), (0, 15)])
    bucket(b16 + "A", 900, [(0,), (16,), (15, 16)])
    bucket(b64, 1000, [(0,), (63,), (0, 63), (0, 1, 63)])
    bucket(b64 + "A", 900, EDGE_PLACES)
    bucket(b128, 800, EDGE_PLACES)
    bucket(b129, 700, [(5,)])
    counted = ranked(entries)
    at = {}
    for k, s in enumerate(inserts(counted)):
        at.setdefault(s, k)
    assert {len(s) for s in at} == {0, 1, 16, 17, 64, 65, 128, 129}
    empty = [k for k, s in enumerate(inserts(counted)) if s == ""]
    assert len(empty) == 2
    expect = {at[c]: (at[h], nsub) for c, h, nsub in kids if len(h) <= MAX_JUNCTION}
    for D in (1, 2):
        _, stats, root = expected_merge(counted, ts, D, 10)
        assert stats["out_of_reach"] == 2
        assert all(root[c] == (h if nsub <= D else c) for c, (h, nsub) in expect.items())
        assert sum(1 for _, nsub in expect.values() if nsub == 3) >= 5
        for R in (1, 10):          # two entries of an empty junction are distance 0 apart
            assert expected_merge(counted, ts, D, R)[2][empty[1]] == empty[0]
    assert int(root[at[sub(b129, 5)]]) == at[sub(b129, 5)]
    return counted, expect


U64 = (1 << 64) - 1


def big_counts(ts):
    """List 2h: [(name, table, D, R, expected root_of or None)] with counts and ratios up to 2^64 - 1."""
    assert full_anchors(ts)
    rng = np.random.default_rng(64)
    X = random_bases(rng, 40)
    cases = []
    # three entries one substitution apart (the same place) with 2^64 - 11, 1 and 2 reads, as given and in rank order
    three = table([bare(1, 2, X, U64 - 10, 0), bare(1, 2, sub(X, 9, 1), 1, 1), bare(1, 2, sub(X, 9, 2), 2, 2)])
    in_rank = ranked([bare(1, 2, X, U64 - 10, 0), bare(1, 2, sub(X, 9, 1), 1, 1), bare(1, 2, sub(X, 9, 2), 2, 2)])
    for R, roots in ((U64 - 10, [0, 0, 2]), (U64 - 9, [0, 1, 2]), (1 << 63, [0, 0, 2]), (1 << 62, [0, 0, 0])):
        cases.append((f"three-R{R}", three, 1, R, roots))
        cases.append((f"ranked-R{R}", in_rank, 1, R, [0, 0 if roots[2] == 0 else 1, 0 if roots[1] == 0 else 2]))
    # a tree whose total is exactly 2^64 - 1
    full = ranked([bare(1, 2, X, U64 - 10, 0), bare(1, 2, sub(X, 3), 7, 1), bare(1, 2, sub(X, 30), 3, 2)])
    assert int(expected_merge(full, ts, 1, 10)[0]["count"][0]) == U64
    cases.append(("total-2^64-1", full, 1, 10, [0, 0, 0]))
    # 2^40 and 2^32 +- 1 in one bucket at R = 10: the ratio's edge in 64 bits, and more than 2^32 reads moved
    A, B, E = (random_bases(rng, 40) for _ in range(3))
    p32, m32 = (1 << 32) + 1, (1 << 32) - 1
    wide = ranked([bare(1, 2, E, 1 << 40, 0), bare(1, 2, A, 10 * p32, 1), bare(1, 2, B, 10 * p32 - 1, 2), bare(1, 2, sub(A, 4), p32, 3),
                   bare(1, 2, sub(B, 4), p32, 4), bare(1, 2, sub(E, 4), m32, 5)])
    out, stats, root = expected_merge(wide, ts, 1, 10)
    assert root.tolist() == [0, 1, 2, 1, 4, 0] and stats["reads_moved"] == 1 << 33
    assert out["count"].tolist() == [(1 << 40) + m32, 11 * p32, 10 * p32 - 1, p32]
    cases.append(("wide", wide, 1, 10, root.tolist()))
    # two roots whose totals tie above 2^32: the tree's first ordinal decides, against the input's rank order
    tie = ranked([bare(1, 2, A, (1 << 33) + 5, 4), bare(1, 2, B, 1 << 33, 9), bare(1, 2, sub(B, 11), 5, 3)])
    out, stats, root = expected_merge(tie, ts, 1, 10)
    assert root.tolist() == [0, 1, 1] and out["count"].tolist() == [(1 << 33) + 5] * 2 and out["first"].tolist() == [3, 4]
    assert inserts(out) == [B, A]
    cases.append(("tie", tie, 1, 10, root.tolist()))
    for name, counted, D, R, roots in cases:
        assert expected_merge(counted, ts, D, R)[2].tolist() == roots, name
    return cases


def zero_counts(ts):
    """List 2i.  count_c = 0 makes an entry the child of any entry within distance (0 <= count_p / R): a head, a zero-count
    entry one substitution from it and one far from everything."""
    assert full_anchors(ts)
    rng = np.random.default_rng(9)
    X = random_bases(rng, 40)
    counted = ranked([bare(1, 2, X, 100, 0), bare(1, 2, sub(X, 17), 0, 1), bare(1, 2, random_bases(rng, 40), 0, 2)])
    for D, R in ((1, 10), (2, 1), (1, U64)):
        _, stats, root = expected_merge(counted, ts, D, R)
        assert root.tolist() == [0, 0, 2] and stats["reads_moved"] == 0 and stats["merged"] == 1
    return counted


def primitive_defects(ts, pairs=300):
    """List 2j.  2 * pairs entries (a parent of 2000 .. reads and its child of 1 .. 9, one substitution apart, 30-base inserts,
    over three gene pairs) in which a few entries carry what dcrx_merge_parents_device's rules call out of reach.  Returns
    (what the device gets: the table, with `text_bytes`; the same table with those entries' inserts turned to N, for the
    contract; the defect ranks)."""
    assert full_anchors(ts)
    rng = np.random.default_rng(606)
    n_v, n_j = len(ts.v_regions), len(ts.j_regions)
    entries = []
    for k in range(pairs):
        s = random_bases(rng, 30)
        v, j = 1 + k % 3, 2
        entries += [bare(v, j, s, 2000 + pairs - k, 2 * k), bare(v, j, sub(s, int(rng.integers(0, 30))), 1 + k % 9, 2 * k + 1)]
    clean = ranked(entries)
    n = len(entries)
    dev = {f: np.array(x, copy=True) if isinstance(x, np.ndarray) else x for f, x in clean.items()}
    text_bytes = len(clean["ins_text"]) - 1          # the last entry's insert leaves the text by one byte
    dev["v"][5], dev["v"][100], dev["j"][255] = n_v, 65535, n_j
    dev["ins_off"][257] = text_bytes + 5          # entry 256 runs past the text, entry 257 goes backwards
    dev["ins_off"][451] = 0          # entry 450 goes backwards; entry 451 is then [0, 452 * 30): longer than any junction
    dev["text_bytes"] = text_bytes
    bad = [5, 100, 255, 256, 257, 450, 451, n - 1]
    text = bytearray(clean["ins_text"])
    for k in bad:
        text[30 * k:30 * k + 30] = b"N" * 30
    contract = dict(clean, ins_text=bytes(text))
    for D, R in ((1, 10), (2, 1)):
        parent, reach = expected_parents(contract, ts, D, R)
        assert [k for k in range(n) if not reach[k]] == bad and all(parent[k] == k for k in bad)
        assert sum(1 for k in range(n) if parent[k] != k) >= pairs - len(bad)
        # defects stand among parents and among children: a child of a defect parent stays alone
        was = expected_parents(clean, ts, D, R)[0]
        assert sum(1 for k in range(n) if was[k] in bad and was[k] != k) >= 3 and sum(1 for k in bad if was[k] != k) >= 2
    return dev, contract, bad


def short_window_mix(ts):
    """List 1g, for a tag set whose V 1 is 20 bases, whose J 1 is 17 bases and whose V 2 has an unclean window: deletions up
    to and one beyond either short window, a chain, the substitution the deletion walk turned into a longer insert, and
    entries on the unclean V."""
    assert len(ts.v_regions[1]) == 20 and len(ts.j_regions[1]) == 17 and not set(ts.v_regions[2].upper()[-ANCHOR:]) <= ACGT
    A = "ACGTTGCAAGGT"
    Vr = ts.v_regions[3].upper()
    vend = Vr[len(Vr) - 3 - 1]          # the germline base a child with vdel 4 gave up
    rows = [(1, 1, 20, 17, A, 500), (1, 1, 20, 17, sub(A, 4), 5),          # both windows deleted whole: the insert alone
            (1, 1, 21, 17, A, 4), (1, 1, 20, 18, A, 3),          # one beyond either window: out of reach
            (1, 1, 3, 2, A, 400), (1, 1, 3, 2, sub(A, 0), 4), (1, 0, 20, 0, A, 300), (1, 0, 20, 0, sub(A, 11), 3),
            (0, 1, 0, 17, A, 200), (0, 1, 0, 17, sub(A, 5), 2), (0, 1, 0, 16, sub(A, 5), 2),
            (2, 0, 3, 2, A, 100), (2, 0, 3, 2, sub(A, 1), 1),          # the unclean V: out of reach
            (0, 0, 3, 2, A, 1000), (0, 0, 3, 2, sub(A, 4), 50), (0, 0, 3, 2, subs(A, (4, 7)), 2),          # a chain
            (3, 0, 3, 0, A, 600), (3, 0, 4, 0, BASES[(BASES.index(vend) + 1) % 4] + A, 6)]
    counted = ranked([r + (k,) for k, r in enumerate(rows)])
    key = [tuple(x) for x in zip(counted["v"].tolist(), counted["j"].tolist(), counted["vdel"].tolist(), counted["jdel"].tolist(),
                                 inserts(counted))]
    at = {k: i for i, k in enumerate(key)}
    _, stats, root = expected_merge(counted, ts, 1, 10)
    assert stats["out_of_reach"] == 4 and stats["merged"] == 7 and stats["longest_chain"] == 2
    for child, head in ((1, 0), (5, 4), (7, 6), (9, 8), (14, 13), (15, 13), (17, 16)):
        assert root[at[rows[child][:5]]] == at[rows[head][:5]]
    assert root[at[rows[10][:5]]] == at[rows[10][:5]]          # one J base more: another length
    return counted
