"""What the weighted `match` tests share (include/dcrx.h "match, weighted"): the contract as plain Python that shares no method
with the kernel — all pairs, the gapped string built literally for every p in 0 .. la and summed over the counted positions —, a
numpy form of the same literal minimum for larger tables, the stand-in for the native call, the file's text, the constructed
lists — each with its premise asserted on the Python result, before any device call — and the host build of the walk
(tests/host_cdr3wmatch).  The lists reuse the constructors of tests/cdr3_match_util.py."""
import ctypes as C
import os
import random

import numpy as np

from decombinator_amd import _native as nat

from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_cdr3wmatch", "build", "libcdr3wmatch_host.so")
MAX_LEN = 32
AMINO = cnu.AMINO
Case = mu.Case


# ---- the contract ----

def letters(s: bytes) -> bool:
    return all(0x41 <= b <= 0x5A for b in s)


def in_reach(s: bytes) -> bool:
    """The network's rule, and under this metric letters alone."""
    return 1 <= len(s) <= MAX_LEN and letters(s)


def gap_sum(a: bytes, b: bytes, p: int, cost) -> int:
    """The sum for ONE gap position p: a (the shorter) with len(b) - len(a) gap marks put in behind its first p residues,
    written out, against b; a residue of a counts when its position in a is ntrim .. la - ctrim - 1."""
    la, d = len(a), len(b) - len(a)
    gapped = [(x, i) for i, x in enumerate(a[:p])] + [None] * d + [(x, p + i) for i, x in enumerate(a[p:])]
    assert len(gapped) == len(b)
    total = 0
    for g, y in zip(gapped, b):
        if g is not None and cost.ntrim <= g[1] < la - cost.ctrim:
            total += int(cost.sub[g[0] & 31, y & 31])
    return total


def dist(a: bytes, b: bytes, cost) -> int:
    """The weighted distance of two strings of letters: the literal minimum over every p."""
    if len(a) > len(b):
        a, b = b, a
    d = len(b) - len(a)
    return d * cost.gap + min(gap_sum(a, b, p, cost) for p in (range(len(a) + 1) if d else (0,)))


_memo = {}


def dist_memo(a: bytes, b: bytes, cost) -> int:
    key = (a, b, cost.gap, cost.ntrim, cost.ctrim, np.asarray(cost.sub).tobytes())
    if key not in _memo:
        _memo[key] = dist(a, b, cost)
    return _memo[key]


def _result(case: Case, rows) -> dict:
    """mu._result with the network's reach for the statistics (a node with a non-letter is in the network's reach), and the
    hits' distances."""
    out = mu._result(case, [[j for j, _ in r] for r in rows])
    out["hit_dist"] = np.array([d for r in rows for _, d in r], dtype=np.uint32)
    return out


def expected(case: Case, cost, R: int) -> dict:
    """What nat.cdr3_match_weighted gives, from the contract: every query against every target of its class.  (dist >=
    d * gap, every cell being >= 0: a pair whose lengths alone cost more than R is not summed.)"""
    rows = []
    t_ok = [in_reach(t) for t in case.t_strings]
    for qc, q in zip(case.q_classes, case.q_strings):
        row = []
        if in_reach(q):
            for j, (c, t) in enumerate(zip(case.t_classes, case.t_strings)):
                if c == qc and t_ok[j] and abs(len(q) - len(t)) * cost.gap <= R:
                    d = dist_memo(q, t, cost)
                    if d <= R:
                        row.append((j, d))
        rows.append(row)
    return _result(case, rows)


def _letters_matrix(strings):
    """(n x 32 letter indices, lengths) of strings in reach."""
    m = np.zeros((len(strings), MAX_LEN), dtype=np.int64)
    for k, s in enumerate(strings):
        m[k, :len(s)] = np.frombuffer(s, dtype=np.uint8) & 31
    return m, np.array([len(s) for s in strings], dtype=np.int64)


def group_dist(a, b, la: int, d: int, cost):
    """dist of arrays of pairs of ONE (la, la + d): a (..., la) and b (..., la + d) hold letter indices and broadcast against each
    other.  The same literal minimum as dist(): for every p in 0 .. la the aligned cells of the counted positions are gathered
    and summed, and the smallest sum kept."""
    sub = np.asarray(cost.sub, dtype=np.int32)
    counted = [i for i in range(la) if cost.ntrim <= i < la - cost.ctrim]
    best = None
    for p in (range(la + 1) if d else (0,)):
        total = np.zeros(np.broadcast(a[..., 0:1], b[..., 0:1]).shape[:-1], dtype=np.int32)
        for i in counted:
            total += sub[a[..., i], b[..., i if i < p else i + d]]
        best = total if best is None else np.minimum(best, total)
    return d * cost.gap + best


def expected_numpy(case: Case, cost, R: int) -> dict:
    """expected() for larger tables: the pairs of one class, grouped by their two lengths, each group through group_dist."""
    t_in = [j for j, t in enumerate(case.t_strings) if in_reach(t)]
    q_in = [i for i, q in enumerate(case.q_strings) if in_reach(q)]
    tm, tl = _letters_matrix([case.t_strings[j] for j in t_in])
    qm, ql = _letters_matrix([case.q_strings[i] for i in q_in])
    tc, qc = np.array([case.t_classes[j] for j in t_in]), np.array([case.q_classes[i] for i in q_in])
    t_in, q_in = np.array(t_in, dtype=np.int64), np.array(q_in, dtype=np.int64)
    found = []      # (query rank, target rank, distance) arrays
    for lq in np.unique(ql).tolist():
        for lt in np.unique(tl).tolist():
            la, d = min(lq, lt), abs(lq - lt)
            if d * cost.gap > R:
                continue
            qi, tj = np.flatnonzero(ql == lq), np.flatnonzero(tl == lt)
            pq, pt = np.nonzero(qc[qi][:, None] == tc[tj][None, :])
            if not len(pq):
                continue
            qs, ts = qm[qi[pq]], tm[tj[pt]]
            dd = group_dist(*((qs, ts) if lq <= lt else (ts, qs)), la, d, cost)
            keep = dd <= R
            found.append((q_in[qi[pq[keep]]], t_in[tj[pt[keep]]], dd[keep]))
    rows = [[] for _ in case.q_strings]
    if found:
        qa, ta, da = (np.concatenate(x) for x in zip(*found))
        order = np.lexsort((ta, qa))
        for i, j, d in zip(qa[order].tolist(), ta[order].tolist(), da[order].tolist()):
            rows[i].append((j, d))
    return _result(case, rows)


def assert_same(got: dict, want: dict, what=""):
    """A nat.cdr3_match_weighted result against the contract: the statistics and every array, the distances too, exactly."""
    mu.assert_same(got, want, what)
    assert np.array_equal(np.asarray(got["hit_dist"], dtype=np.uint64), np.asarray(want["hit_dist"], dtype=np.uint64)), (what, "hit_dist")


# ---- costs ----

def default_cost(gap=12, ntrim=3, ctrim=2):
    return nat.Cdr3Cost.default(gap, ntrim, ctrim)


def random_table(seed: int, top: int = 255) -> np.ndarray:
    """A valid table: symmetric, zero on the diagonal, cells 0 .. top (a few of them 0 off the diagonal)."""
    rnd = random.Random(seed)
    sub = np.zeros((32, 32), dtype=np.uint8)
    for x in range(1, 27):
        for y in range(1, x):
            sub[x, y] = sub[y, x] = 0 if rnd.random() < 0.05 else rnd.randrange(top + 1)
    return sub


def random_cost(seed: int, gap: int, ntrim: int, ctrim: int, top: int = 255):
    return nat.Cdr3Cost(random_table(seed, top), gap, ntrim, ctrim)


def unit_cost():
    """Every substitution 1, a gap 1, no trims."""
    sub = np.zeros((32, 32), dtype=np.uint8)
    sub[1:27, 1:27] = 1
    sub[np.arange(32), np.arange(32)] = 0
    return nat.Cdr3Cost(sub, 1, 0, 0)


# ---- the native call, its stand-in, the file's text ----

def native_match(case: Case, cost, R: int) -> dict:
    """nat.Cdr3Index and nat.cdr3_match_weighted on a case (GPU)."""
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        return nat.cdr3_match_weighted(index, *q_args, cost, R)
    finally:
        index.close()


def brute_force_native(calls=None):
    """What stands in for nat.cdr3_match_weighted: the contract, in the native function's shape."""
    def cdr3_match_weighted(index, classes, off, text, weights, cost, radius):
        strings = cnu.node_strings(off, text)
        if calls is not None:
            calls.append((index, np.asarray(classes).tolist(), strings, np.asarray(weights).tolist(), cost, int(radius)))
        return expected(Case(index.classes, index.strings, classes, strings, weights), cost, int(radius))
    return cdr3_match_weighted


def matches_text(v_calls, j_calls, case: Case, result: dict, db_header, db_lines, cost) -> bytes:
    """The `.cdr3_matches.tsv` text under the weighted metric: one line per hit by (query, target)."""
    lines = [b"\t".join([c.encode() for c in nat.CDR3_MATCH_COLUMNS] + [b"db_" + h for h in db_header])]
    off = result["hit_off"]
    for i, q in enumerate(case.q_strings):
        for j in np.asarray(result["hit"])[int(off[i]):int(off[i + 1])].tolist():
            lines.append(b"\t".join([str(i).encode(), v_calls[i].encode("latin-1"), j_calls[i].encode("latin-1"), q,
                                     str(case.weights[i]).encode(), str(j).encode(), str(dist(q, case.t_strings[j], cost)).encode(),
                                     db_lines[j]]))
    return b"\n".join(lines) + b"\n"


# ---- the constructed lists: name -> (case, cost, R), each with its premise asserted on the Python result ----

def _s(x) -> bytes:
    return x if isinstance(x, bytes) else x.encode("latin-1")


def _degrees(case, cost, R):
    return expected(case, cost, R)["degree"].tolist()


def single_pairs():
    """One node a side: equal; differing in trimmed positions alone at R = 0; one conservative substitution (I-V, 3 by default)
    with R at its cost and one below."""
    cost = default_cost()
    out = {}
    equal = Case([0], ["CASSIRSSYEQYF"], [0], ["CASSIRSSYEQYF"])
    trimmed = Case([0], ["CASSIRSSYEQYF"], [0], ["WWWSIRSSYEQWW"])
    near = Case([0], ["CASSIRSSYEQYF"], [0], ["CASSVRSSYEQYF"])
    assert dist(b"CASSIRSSYEQYF", b"WWWSIRSSYEQWW", cost) == 0 and dist(b"CASSIRSSYEQYF", b"CASSVRSSYEQYF", cost) == 3
    assert _degrees(equal, cost, 0) == [1] and _degrees(trimmed, cost, 0) == [1]
    assert _degrees(near, cost, 3) == [1] and _degrees(near, cost, 2) == [0]
    out["equal_R0"], out["trimmed_only_R0"] = (equal, cost, 0), (trimmed, cost, 0)
    out["conservative_at_cost"], out["conservative_one_below"] = (near, cost, 3), (near, cost, 2)
    out["no_nodes"] = (Case([], [], [], []), cost, 24)
    out["no_targets"] = (Case([], [], [0], ["CASSF"]), cost, 24)
    out["no_queries"] = (Case([0], ["CASSF"], [], []), cost, 24)
    return out


LENGTHS = (1, 2, 4, 5, 6, 8, 9, 16, 17, 31, 32, 33)
EDGES = (3, 4, 7, 8, 15, 16, 27, 28, 31)


def _base(L: int) -> bytes:
    return bytes(AMINO[(3 * p + p // 7) % 20].encode()[0] for p in range(L))


def every_position(L: int, cost=None, longer: str = "target"):
    """One target of L letters against: itself; a substitution at EVERY position (counted ones cost, uncounted ones are free);
    pairs of substitutions at the dword edges; and (L > 1) every deletion of one residue, so that the two sides differ in length
    in the direction `longer` says.  R is one radical substitution's cost: a counted single substitution hits, two do not
    unless one is free."""
    cost = cost or default_cost()
    base = _base(L)
    other = lambda b: b"W" if b not in b"WFY" else b"D"      # (12 from every base letter under the default table)
    qs = [base] + [base[:p] + other(base[p:p + 1]) + base[p + 1:] for p in range(L)]
    edges = [p for p in EDGES if p < L]
    qs += [base[:a] + other(base[a:a + 1]) + base[a + 1:b] + other(base[b:b + 1]) + base[b + 1:] for a in edges for b in edges if a < b]
    if L > 1:
        qs += [base[:p] + base[p + 1:] for p in range(L)]
    case = Case([0], [base], [0] * len(qs), qs)
    if longer == "query":
        case = case.swapped()
    R = 12
    if L <= MAX_LEN:
        want = expected(case, cost, R)
        counted = [cost.ntrim <= p < L - cost.ctrim for p in range(L)]
        singles = [dist(base, q, cost) for q in qs[1:L + 1]]
        assert singles == [12 if c else 0 for c in counted], (L, singles)
        assert want["stats"]["hits"] >= 1 + L                      # itself and every single substitution
        if any(counted[a] and counted[b] for a in edges for b in edges if a < b):
            assert want["stats"]["hits"] < len(qs)                 # two counted substitutions pass R
    else:
        assert expected(case, cost, 65535)["stats"]["hits"] == 0      # 33 letters: out of reach
    return case, cost, R


def gap_positions():
    """Length differences d = 1, 2 and the largest the window allows (R // gap), with the best gap position the first counted
    one, the last counted one, strictly inside, and one pair where two positions tie; and la <= ntrim + ctrim with d > 0."""
    cost = default_cost()
    out = {}
    a = b"CASSLAPGATNEKLF"                    # la = 15: counted 3 .. 12, the gap counts between p = 3 and p = 13
    best_p = lambda x, y: [gap_sum(x, y, p, cost) for p in range(len(x) + 1)]
    for d, R in ((1, 24), (2, 24), (4, 48)):
        ins = b"WHWH"[:d]
        for name, p in (("first", 3), ("inside", 8), ("last", 13)):
            b = a[:p] + ins + a[p:]
            sums = best_p(a, b)
            assert sums[p] == 0 and min(sums) == 0 and dist(a, b, cost) == d * 12
            if name == "inside":
                assert sums[3] > 0 and sums[13] > 0
            case = Case([0, 0], [b, a], [0, 0], [a, b])
            assert _degrees(case, cost, R) == [2, 2] and _degrees(case, cost, d * 12 - 1) == [1, 1]
            out[f"gap_d{d}_{name}"] = (case, cost, R)
        assert (R // cost.gap == d) or d < 4
    # p < ntrim costs what p = ntrim costs: the first counted position is the best only as the end of the plateau
    b = b"W" + a
    sums = best_p(a, b)
    assert len(set(sums[:4])) == 1 and sums[0] == min(sums)
    out["gap_plateau_front"] = (Case([0], [b], [0], [a]), cost, 24 + sums[0])
    # a tie: in a run of one letter the gap may stand anywhere in it
    t = b"CASSGGGGGGNEKLF"
    u = b"CASSGGGGGGGNEKLF"
    sums = best_p(t, u)
    assert sums.count(min(sums)) >= 7 and dist(t, u, cost) == 12
    out["gap_tie"] = (Case([0], [u], [0], [t]), cost, 12)
    # nothing counted: la <= ntrim + ctrim, so the distance is the gap's alone
    for la in (1, 4, 5):
        short, long_ = b"CASSF"[:la], b"WWWWWWW"[:la + 2]
        assert dist(short, long_, cost) == 24
        case = Case([0, 0], [long_, short], [0, 0], [short, long_])
        assert _degrees(case, cost, 24) == [2, 2] and _degrees(case, cost, 23) == [1, 1]
        out[f"nothing_counted_{la}"] = (case, cost, 24)
        out[f"nothing_counted_{la}_below"] = (case, cost, 23)
    return out


def large_sums():
    """Cells of 255 and no trims: 32 substitutions add up to 8 160 > 2^12, and 31 gapped positions at 255 to 7 905; R = 65535
    takes everything, R = 8 159 leaves out exactly the pairs at 8 160."""
    sub = np.zeros((32, 32), dtype=np.uint8)
    sub[1:27, 1:27] = 255
    sub[np.arange(32), np.arange(32)] = 0
    cost = nat.Cdr3Cost(sub, 255, 0, 0)
    a, b = b"A" * 32, b"C" * 32
    qs = [a, b"A" * 20 + b"C" * 12, b"A", b"C" * 17]
    case = Case([0, 0], [b, b"C"], [0] * 4, qs)
    assert dist(a, b, cost) == 8160 > 1 << 12 and dist(b"A", b, cost) == 7905 + 255 and dist(b"C", b, cost) == 7905
    assert _degrees(case, cost, 65535) == [2, 2, 2, 2] and _degrees(case, cost, 8159) == [0, 2, 1, 2]
    return {"sums_past_2_12": (case, cost, 65535), "sums_one_below": (case, cost, 8159)}


def trims():
    """ntrim = ctrim = 0: every position counts; ntrim = ctrim = 16: nothing of any string counts, so every pair of a class
    within the length window is a hit at its gap's price."""
    rnd = random.Random(11)
    strings = ["".join(rnd.choice(AMINO) for _ in range(L)) for L in (1, 7, 15, 16, 17, 31, 32, 32, 12, 13)]
    case = Case([0] * len(strings), strings, [0] * len(strings), strings[::-1])
    none, all_ = default_cost(12, 0, 0), default_cost(12, 16, 16)
    want = expected(case, all_, 24)
    assert all(d % 12 == 0 for d in want["hit_dist"].tolist()) and want["stats"]["hits"] > len(strings)
    own = expected(case, none, 24)
    assert own["stats"]["queries_hit"] == len(strings) and 0 in own["hit_dist"].tolist() and own["stats"]["hits"] < want["stats"]["hits"]
    return {"trim_0_0": (case, none, 24), "trim_16_16": (case, all_, 24)}


def non_letters():
    """Nodes with a byte outside A .. Z — lower case, `*`, 0x00, 0x80, `_` — mixed into one full class of 600 targets, on the first
    and last slot of the tiles of 256 (ranks 0, 255, 256, 511) and at the end, and among the queries; a node out of the
    network's reach (empty, 33 letters) on a tile's first and last slot of a second class."""
    cost = default_cost()
    bad = {0: b"cASSAAAEQYF", 255: b"CASS*AAEQYF", 256: b"CASSA\x00AEQYF", 511: b"CASSA\x80AEQYF", 599: b"CASS_AAEQYF", 300: b"CASSAAAEQYf"}
    ts = [bad.get(i, mu.code(i).encode()) for i in range(600)]
    tc = [4] * 600
    far = {0: b"", 255: b"A" * 33, 256: b"", 299: b"C" * 40}
    ts += [far.get(i, mu.code(i).encode()) for i in range(300)]
    tc += [9] * 300
    qs = [mu.code(i).encode() for i in (0, 1, 255, 256, 300, 511, 599)] + list(bad.values()) + [b"", b"A" * 33]
    qc = [4] * (7 + len(bad)) + [9, 9]
    qs += [mu.code(i).encode() for i in (0, 255, 256, 299)]
    qc += [9] * 4
    case = Case(tc, ts, qc, qs)
    want = expected(case, cost, 24)
    assert not (set(want["hit"].tolist()) & set(bad)) and want["degree"][7:7 + len(bad) + 2].tolist() == [0] * (len(bad) + 2)
    assert all(want["degree"][k] > 0 for k in range(7)) and want["stats"]["targets_out_of_reach"] == 4
    assert not (set(want["hit"].tolist()) & {600 + k for k in far})
    return {"non_letters": (case, cost, 24), "non_letters_swapped": (case.swapped(), cost, 24)}


def tails(case: Case) -> Case:
    """The case with the last 0 .. 2 letters of every string cut off by its rank: lengths that differ inside a bucket."""
    cut = lambda s, k: s[:len(s) - k % 3] if len(s) > 4 else s
    return Case(case.t_classes, [cut(s, k) for k, s in enumerate(case.t_strings)], case.q_classes,
                [cut(s, 2 * k + 1) for k, s in enumerate(case.q_strings)], case.weights)


def buckets():
    """The walk's lists of tests/cdr3_match_util.py — one bucket of 255 / 256 / 257 / 513 targets or queries, 1 500 queries in six
    blocks, buckets missing on either side, classes that differ in one bit (bit 31 too) — with lengths mixed inside a bucket."""
    cost = default_cost()
    out = {}
    for n in (255, 256, 257, 513):
        out[f"targets_{n}"] = (tails(mu.one_bucket(n, 6)), cost, 24)
        out[f"queries_{n}"] = (tails(mu.one_bucket(40, n)), cost, 24)
    out["queries_1500"] = (tails(mu.one_bucket(40, 1500)), cost, 24)
    for lack in ("t_first", "t_last", "q_first", "q_last"):
        out[f"gaps_{lack}"] = (tails(mu.bucket_gaps(lack)), cost, 24)
    for k, pair in enumerate(cnu.CLASS_BIT_PAIRS):
        out[f"class_bits_{k}"] = (mu.class_bits(pair, n_out=5 * k), cost, 12)
    for name, (case, c, R) in out.items():
        want = expected(case, c, R)
        assert want["stats"]["hits"] > 0, name
        if name.startswith(("targets_", "queries_")):
            assert len({int(d) for d in want["hit_dist"]}) >= 3 and any(len(case.q_strings[i]) != len(case.t_strings[j]) for i in range(
                len(case.q_strings)) for j in want["hit"][int(want["hit_off"][i]):int(want["hit_off"][i + 1])].tolist()), name
    return out


_constructed = None
# the lists' names, known without building them (constructed() checks them)
NAMES = (["equal_R0", "trimmed_only_R0", "conservative_at_cost", "conservative_one_below", "no_nodes", "no_targets", "no_queries"]
         + [f"length_{L}_{longer}_longer" for L in LENGTHS for longer in ("target", "query")]
         + [f"gap_d{d}_{where}" for d in (1, 2, 4) for where in ("first", "inside", "last")] + ["gap_plateau_front", "gap_tie"]
         + [f"nothing_counted_{la}{below}" for la in (1, 4, 5) for below in ("", "_below")]
         + ["sums_past_2_12", "sums_one_below", "trim_0_0", "trim_16_16", "non_letters", "non_letters_swapped"]
         + [f"{side}_{n}" for n in (255, 256, 257, 513) for side in ("targets", "queries")] + ["queries_1500"]
         + [f"gaps_{lack}" for lack in ("t_first", "t_last", "q_first", "q_last")]
         + [f"class_bits_{k}" for k in range(len(cnu.CLASS_BIT_PAIRS))])


def constructed() -> dict:
    """The lists the host walk and the device are pinned on: name -> (Case, cost, R).  Built once."""
    global _constructed
    if _constructed is None:
        out = {}
        out.update(single_pairs())
        for L in LENGTHS:
            out[f"length_{L}_target_longer"] = every_position(L, longer="target")
            out[f"length_{L}_query_longer"] = every_position(L, longer="query")
        out.update(gap_positions())
        out.update(large_sums())
        out.update(trims())
        out.update(non_letters())
        out.update(buckets())
        assert sorted(out) == sorted(NAMES)
        _constructed = out
    return _constructed


# ---- the walk and the pair test on the host (tests/host_cdr3wmatch) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_cdr3wmatch")])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        _host.cdr3wmatch_host_within.restype = u32
        _host.cdr3wmatch_host_within.argtypes = [vp, u32, vp, u32, vp, u32, u32, u32, u32]
        _host.cdr3wmatch_host_within_many.restype = None
        _host.cdr3wmatch_host_within_many.argtypes = [u64, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp]
        _host.cdr3wmatch_host_within_grid.restype = None
        _host.cdr3wmatch_host_within_grid.argtypes = [u64, vp, u32, u64, vp, u32, vp, u32, u32, u32, u32, vp]
        _host.cdr3wmatch_host_letters.restype = C.c_int
        _host.cdr3wmatch_host_letters.argtypes = [vp, u32]
        _host.cdr3wmatch_host_match.restype = u64
        _host.cdr3wmatch_host_match.argtypes = [u64, vp, vp, vp] * 2 + [vp, u32, u32, u32, u32] + [vp, vp, vp, vp, u64]
    return _host


def _cost_args(cost):
    sub = np.ascontiguousarray(cost.sub, dtype=np.uint8)
    return sub, [sub.ctypes.data, cost.gap, cost.ntrim, cost.ctrim]


def host_within(a: bytes, b: bytes, cost, R: int) -> int:
    """weighted_within of the shared header: a as the lane's own string, b as the staged one."""
    sub, args = _cost_args(cost)
    pa, pb = (np.frombuffer(x + b"\0" * (MAX_LEN + 1 - len(x)), np.uint8) for x in (a, b))
    return int(host_lib().cdr3wmatch_host_within(pa.ctypes.data, len(a), pb.ctypes.data, len(b), *args, R))


def host_within_many(pairs, cost, R: int):
    sub, args = _cost_args(cost)
    n = len(pairs)
    A, B = np.zeros((n, MAX_LEN), np.uint8), np.zeros((n, MAX_LEN), np.uint8)
    la, lb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for k, (a, b) in enumerate(pairs):
        A[k, :len(a)], B[k, :len(b)] = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
        la[k], lb[k] = len(a), len(b)
    out = np.zeros(n, np.uint32)
    host_lib().cdr3wmatch_host_within_many(n, A.ctypes.data, la.ctypes.data, B.ctypes.data, lb.ctypes.data, *args, R, out.ctypes.data)
    return out


def host_within_grid(A, la: int, B, lb: int, cost, R: int):
    """weighted_within of every row of A (n_a x 32 bytes, la each: the own strings) against every row of B (lb each)."""
    sub, args = _cost_args(cost)
    A, B = np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8)
    out = np.zeros((len(A), len(B)), np.uint32)
    host_lib().cdr3wmatch_host_within_grid(len(A), A.ctypes.data, la, len(B), B.ctypes.data, lb, *args, R, out.ctypes.data)
    return out


def host_letters(s: bytes) -> bool:
    p = np.frombuffer(s + b"\0" * (MAX_LEN + 1 - len(s)), np.uint8)
    return bool(host_lib().cdr3wmatch_host_letters(p.ctypes.data, len(s)))


def host_match(case: Case, cost, R: int):
    """(degree, hit_off, hit, hit_dist) of the host walk."""
    (tc, t_off, t_text), (qc, q_off, q_text, _) = mu.native_args(case)
    tt, qt = (np.frombuffer(x + b"\0", np.uint8) for x in (t_text, q_text))
    sub, cargs = _cost_args(cost)
    m_q = len(qc)
    degree, hit_off = np.zeros(max(m_q, 1), np.uint32), np.zeros(m_q + 1, np.uint64)
    args = [len(tc), tc.ctypes.data, t_off.ctypes.data, tt.ctypes.data, m_q, qc.ctypes.data, q_off.ctypes.data, qt.ctypes.data, *cargs, R]
    one = np.zeros(1, np.uint32)
    need = host_lib().cdr3wmatch_host_match(*args, degree.ctypes.data, hit_off.ctypes.data, one.ctypes.data, one.ctypes.data, 0)
    hit, hd = np.zeros(max(need, 1), np.uint32), np.zeros(max(need, 1), np.uint32)
    assert host_lib().cdr3wmatch_host_match(*args, degree.ctypes.data, hit_off.ctypes.data, hit.ctypes.data, hd.ctypes.data, need) == need
    return degree[:m_q], hit_off, hit[:need], hd[:need]
