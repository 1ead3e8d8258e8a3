"""What the weighted CDR3 network tests share (include/dcrx.h "the CDR3 network, weighted"): the contract from Python that shares
no method with the kernel — every pair's distance from tests/cdr3_wmatch_util.py's dist (the gapped string built literally for
every p) or, for larger tables, its numpy form group_dist, a node never paired with itself, clusters from a plain union-find
over all pairs —, the stand-in for the native call, the edges file's text, the constructed lists — each with its premise asserted
on the Python result, before any device call — and the host build of the walk (tests/host_cdr3wnet)."""
import ctypes as C
import os
import random

import numpy as np

from decombinator_amd import _native as nat

from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_cdr3wnet", "build", "libcdr3wnet_host.so")
MAX_LEN = 32
AMINO = cnu.AMINO


class Nodes:
    """Nodes (class, string, weight) in rank order."""

    def __init__(self, classes, strings, weights=None):
        self.classes, self.strings = [int(c) for c in classes], cnu.as_bytes(strings)
        assert len(self.classes) == len(self.strings)
        self.weights = [1 + (5 * k) % 13 for k in range(len(self.strings))] if weights is None else [int(w) for w in weights]

    def __len__(self):
        return len(self.strings)


# ---- the contract ----

def _network(nodes: Nodes, rows):
    """(result, stats) from every node's neighbours (rank, distance) in ascending rank: the CSR, and the clusters by a union-find
    over all pairs whose root is the smallest rank."""
    m = len(nodes)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, row in enumerate(rows):
        for j, _ in row:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = [find(i) for i in range(m)]
    heads = sorted(set(root))
    slot = {h: r for r, h in enumerate(heads)}
    size, weight = [0] * len(heads), [0] * len(heads)
    for i in range(m):
        size[slot[root[i]]] += 1
        weight[slot[root[i]]] += nodes.weights[i]
    degree = [len(r) for r in rows]
    adj_off = np.zeros(m + 1, dtype=np.uint64)
    if m:
        adj_off[1:] = np.cumsum(degree)
    result = {"degree": np.array(degree, dtype=np.uint32), "cluster_of": np.array([slot[r] for r in root], dtype=np.uint32),
              "cluster_head": np.array(heads, dtype=np.uint32), "cluster_size": np.array(size, dtype=np.uint32),
              "cluster_weight": np.array(weight, dtype=np.uint64), "adj_off": adj_off,
              "adj": np.array([j for r in rows for j, _ in r], dtype=np.uint32),
              "adj_dist": np.array([d for r in rows for _, d in r], dtype=np.uint32)}
    stats = {"nodes_in": m, "out_of_reach": sum(not 1 <= len(s) <= MAX_LEN for s in nodes.strings), "edges": sum(degree) // 2,
             "clusters_out": len(heads), "singletons": sum(1 for x in size if x == 1), "largest_cluster": max(size, default=0),
             "largest_degree": max(degree, default=0)}
    assert list(stats) == list(nat.CDR3_NETWORK_STATS) and sum(degree) % 2 == 0
    return result, stats


def _rows(nodes: Nodes, hits: dict):
    """Every node's (rank, distance) out of a table-against-itself result of tests/cdr3_wmatch_util.py, itself left out."""
    off, hit, hd = hits["hit_off"], np.asarray(hits["hit"]).tolist(), np.asarray(hits["hit_dist"]).tolist()
    return [[(hit[k], hd[k]) for k in range(int(off[i]), int(off[i + 1])) if hit[k] != i] for i in range(len(nodes))]


def _as_case(nodes: Nodes) -> mu.Case:
    return mu.Case(nodes.classes, nodes.strings, nodes.classes, nodes.strings, nodes.weights)


def expected(nodes: Nodes, cost, R: int):
    """What nat.cdr3_network_weighted gives with want_edges, from the contract: every node against every other node of its
    class, the distance by wu.dist."""
    return _network(nodes, _rows(nodes, wu.expected(_as_case(nodes), cost, R)))


def expected_numpy(nodes: Nodes, cost, R: int):
    """expected() for larger tables: the distances by wu.group_dist."""
    return _network(nodes, _rows(nodes, wu.expected_numpy(_as_case(nodes), cost, R)))


KEYS = ("degree", "cluster_of", "cluster_head", "cluster_size", "cluster_weight")
EDGE_KEYS = ("adj_off", "adj", "adj_dist")


def assert_same(got, want, what=""):
    """(result, stats) of nat.cdr3_network_weighted against the contract: the statistics and every array, exactly."""
    (gr, gs), (wr, ws) = got, want
    assert gs == ws, (what, gs, ws)
    for k in KEYS + (EDGE_KEYS if "adj_off" in gr else ()):
        assert np.array_equal(np.asarray(gr[k], dtype=np.uint64), np.asarray(wr[k], dtype=np.uint64)), (what, k)


def symmetric(result) -> bool:
    """Every adjacency entry stands in the other node's row too, with the same distance."""
    off, adj, dist = result["adj_off"], np.asarray(result["adj"]).tolist(), np.asarray(result["adj_dist"]).tolist()
    pairs = {(i, adj[k]): dist[k] for i in range(len(off) - 1) for k in range(int(off[i]), int(off[i + 1]))}
    return all(pairs.get((j, i)) == d for (i, j), d in pairs.items())


# ---- the native call, its stand-in, the file's text ----

def native(nodes: Nodes, cost, R: int, want_edges=True):
    """nat.cdr3_network_weighted on the nodes (GPU)."""
    off, text = cnu.node_text(nodes.strings)
    return nat.cdr3_network_weighted(np.array(nodes.classes, dtype=np.uint32), off, text, nodes.weights, cost, R, want_edges=want_edges)


def brute_force_native(calls=None):
    """What stands in for nat.cdr3_network_weighted: the contract, in the native function's shape."""
    def cdr3_network_weighted(classes, aa_off, aa_text, weights, cost, radius, want_edges=False):
        strings = cnu.node_strings(aa_off, aa_text)
        if calls is not None:
            calls.append((np.asarray(classes).tolist(), strings, cost, int(radius), bool(want_edges)))
        result, stats = expected(Nodes(classes, strings, weights), cost, int(radius))
        if not want_edges:
            for k in EDGE_KEYS:
                del result[k]
        return result, stats
    return cdr3_network_weighted


def edges_text(strings, result, cost) -> str:
    """The `.cdr3_edges.tsv` text: every edge a < b, ascending by (a, b), with the weighted distance of the two strings."""
    strings = cnu.as_bytes(strings)
    lines = ["\t".join(nat.CDR3_EDGE_COLUMNS)]
    off, adj = result["adj_off"], result["adj"]
    for a in range(len(strings)):
        for b in np.asarray(adj[int(off[a]):int(off[a + 1])]).tolist():
            if a < b:
                lines.append(f"{a}\t{b}\t{wu.dist(strings[a], strings[b], cost)}")
    return "\n".join(lines) + "\n"


_wanted = {}      # name -> the contract's (result, stats) of a constructed list


# ---- the constructed lists: name -> (Nodes, cost, R, numpy), each with its premise asserted on the Python result ----

def code(i: int) -> bytes:
    """String number i: three base-20 digits between fixed ends (two numbers differ in 1 to 3 places) and a tail of 2 + i % 3
    letters — three lengths mixed inside a class."""
    digits, n = "", i
    for _ in range(3):
        digits += AMINO[i % 20]
        i //= 20
    return ("CASS" + digits + "EQYF"[:2 + n % 3]).encode()


def small():
    """No node; one node; two equal strings at R = 0; two strings that differ in trimmed positions alone at R = 0; one
    conservative substitution (I-V, 3 by default) with R at its cost and one below."""
    cost = wu.default_cost()
    a, v, t = b"CASSIRSSYEQYF", b"CASSVRSSYEQYF", b"WWWSIRSSYEQWW"
    assert wu.dist(a, t, cost) == 0 and wu.dist(a, v, cost) == 3
    out = {"no_nodes": (Nodes([], []), cost, 24), "one_node": (Nodes([0], [a]), cost, 24),
           "equal_R0": (Nodes([0, 0], [a, a]), cost, 0), "trimmed_only_R0": (Nodes([0, 0], [a, t]), cost, 0),
           "conservative_at_cost": (Nodes([0, 0], [a, v]), cost, 3), "conservative_one_below": (Nodes([0, 0], [a, v]), cost, 2)}
    degrees = {k: expected(*x)[0]["degree"].tolist() for k, x in out.items()}
    assert degrees == {"no_nodes": [], "one_node": [0], "equal_R0": [1, 1], "trimmed_only_R0": [1, 1], "conservative_at_cost": [1, 1],
                       "conservative_one_below": [0, 0]}
    assert expected(*out["equal_R0"])[0]["adj_dist"].tolist() == [0, 0] and expected(*out["conservative_at_cost"])[1]["clusters_out"] == 1
    return {k: x + (False,) for k, x in out.items()}


SYM_LENGTHS = (1, 4, 5, 8, 9, 16, 17, 31)
SYM_GAPS = (1, 2, 4)


def symmetry(ntrim: int, ctrim: int):
    """Pairs of lengths (L, L + d), L + d <= 32, each pair a class of its own: the longer string is the shorter one with d letters
    put in at the first counted position, at the last one and strictly inside (where the shorter string has such positions; at
    p = 0 otherwise), so that the pair's distance is d * gap and is reached at that place alone; R = d * gap for every pair of
    the list would differ by d, so the list runs at R = 4 * gap and the distance itself is compared.  Either string comes first
    in rank in turn.  -> (Nodes, cost, R, the pairs' (rank of the shorter, rank of the longer, d, place))."""
    cost = wu.default_cost(12, ntrim, ctrim)
    classes, strings, pairs = [], [], []
    for L in SYM_LENGTHS:
        base = wu._base(L)
        for d in SYM_GAPS:
            if L + d > MAX_LEN:
                continue
            lo, hi = ntrim, L - ctrim      # the gap counts from p = lo to p = hi
            places = [("first", lo), ("last", hi), ("inside", (lo + hi) // 2)] if hi - lo >= 2 else [("only", 0)]
            for name, p in places:
                ins = bytes(b"WHWH"[k] if b"WHWH"[k] not in base[max(0, p - 1):p + 1] else ord("P") for k in range(d))
                longer = base[:p] + ins + base[p:]
                sums = [wu.gap_sum(base, longer, q, cost) for q in range(L + 1)]
                assert sums[p] == 0 and wu.dist(base, longer, cost) == d * cost.gap, (L, d, name)
                if name == "inside":
                    assert sums[lo] > 0 and sums[hi] > 0, (L, d, sums)
                elif name == "first":
                    assert sums[hi] > 0, (L, d, sums)
                elif name == "last":
                    assert sums[lo] > 0, (L, d, sums)
                c = len(pairs)
                first_short = c % 2 == 0
                at = len(strings)
                strings += [base, longer] if first_short else [longer, base]
                classes += [c, c]
                pairs.append((at if first_short else at + 1, at + 1 if first_short else at, d, name))
    nodes = Nodes(classes, strings)
    want, stats = expected(nodes, cost, 4 * cost.gap)
    assert want["degree"].tolist() == [1] * len(nodes) and stats["edges"] == len(pairs)
    assert {n for _, _, _, n in pairs} >= {"first", "last", "inside", "only"} and len(pairs) > 40
    return nodes, cost, 4 * cost.gap, pairs


def tiles(n: int, n_classes: int = 1):
    """One class of n nodes code(0 .. n - 1), three lengths mixed: in class order a node's own entry is slot s % 256 of its
    tile — slot 0 and slot 255 occur from 256 nodes on —, and every node has neighbours in every tile.  (n_classes > 1: the
    ranks dealt out over that many classes seven at a time, so that blocks and tiles span class starts.)"""
    nodes = Nodes([7 + i // 7 % n_classes for i in range(n)], [code(i) for i in range(n)])
    cost = wu.default_cost()
    want, stats = _wanted[f"tiles_{n}"] = expected_numpy(nodes, cost, 24)
    assert stats["largest_degree"] > 20 and min(want["degree"].tolist()) > 0 and len(set(want["adj_dist"].tolist())) >= 4
    off, adj = want["adj_off"], want["adj"]
    assert any(len(nodes.strings[i]) != len(nodes.strings[j]) for i in (0, n - 1) for j in adj[int(off[i]):int(off[i + 1])].tolist())
    if n > 256 and n_classes == 1:
        assert 256 in adj[int(off[255]):int(off[256])].tolist() and 255 in adj[int(off[256]):int(off[257])].tolist()
    return nodes, cost, 24


def components():
    """A chain A - B - C with dist(A, C) > R in one cluster; the same strings under a second class, and under a class that
    differs from the first in bit 31 alone, stay apart."""
    cost = wu.default_cost()
    a, b, c = b"CASSIRSSYEQYF", b"CASSWRSSYEQYF", b"CASSWRSDYEQYF"
    assert (wu.dist(a, b, cost), wu.dist(b, c, cost), wu.dist(a, c, cost)) == (12, 12, 24)
    chain = Nodes([0, 0, 0], [c, a, b])
    want, stats = expected(chain, cost, 12)
    assert want["degree"].tolist() == [1, 1, 2] and stats["clusters_out"] == 1 and want["cluster_size"].tolist() == [3]
    out = {"chain": (chain, cost, 12, False)}
    for k, pair in enumerate(cnu.CLASS_BIT_PAIRS):
        classes, strings, which = cnu.class_bit_nodes([code(i) for i in range(60)], pair, n_out=4 * k)
        nodes = Nodes(classes, strings)
        want, stats = expected(nodes, cost, 24)
        assert cnu.no_edge_across(which, want) and stats["edges"] > 60
        heads = want["cluster_head"].tolist()
        assert all(len({which[i] for i in range(len(nodes)) if want["cluster_of"][i] == r}) == 1 for r in range(len(heads)))
        out[f"class_bits_{k}"] = (nodes, cost, 24, False)
    return out


BAD_BYTES = {0: b"cASSAAAEQYF", 255: b"CASS*AAEQYF", 256: b"CASSA\x00AEQYF", 599: b"CASSA\x80AEQYF"}


def reach():
    """A class of 600 nodes with a byte outside A .. Z — lower case, `*`, 0x00, 0x80 — at ranks 0, 255, 256 and last, and 33
    letters at rank 300: degree 0, a cluster of their own, in nobody's row."""
    cost = wu.default_cost()
    strings = [BAD_BYTES.get(i, b"A" * 33 if i == 300 else code(i)) for i in range(600)]
    nodes = Nodes([4] * 600, strings)
    want, stats = _wanted["reach"] = expected_numpy(nodes, cost, 24)
    out = set(BAD_BYTES) | {300}
    assert all(want["degree"][i] == 0 and want["cluster_size"][want["cluster_of"][i]] == 1 for i in out)
    assert not (set(want["adj"].tolist()) & out) and stats["out_of_reach"] == 1 and stats["singletons"] == len(out)
    assert all(want["degree"][i] > 0 for i in (1, 254, 257, 598))
    return {"reach": (nodes, cost, 24, True)}


def costs():
    """Cells of 255 and no trims at R = 65535 and at one below the largest distance (8 160, which four pairs have); trims 0,0 and 16,16; a random table."""
    sub = np.zeros((32, 32), dtype=np.uint8)
    sub[1:27, 1:27] = 255
    sub[np.arange(32), np.arange(32)] = 0
    top = nat.Cdr3Cost(sub, 255, 0, 0)
    strings = [b"A" * 32, b"C" * 32, b"A" * 20 + b"C" * 12, b"A", b"C" * 17, b"C"]
    nodes = Nodes([0] * 6, strings)
    assert wu.dist(strings[0], strings[1], top) == 8160 and wu.dist(b"A", b"C" * 32, top) == 8160
    all_, stats = expected(nodes, top, 65535)
    below, stats_below = expected(nodes, top, 8159)
    assert all_["degree"].tolist() == [5] * 6 and max(all_["adj_dist"].tolist()) == 8160 and stats_below["edges"] == stats["edges"] - 4      # (four pairs at 8 160)
    out = {"cells_255_R65535": (nodes, top, 65535, False), "cells_255_one_below": (nodes, top, 8159, False)}
    rnd = random.Random(11)
    mixed = Nodes([0] * 14, ["".join(rnd.choice(AMINO) for _ in range(L)) for L in (1, 7, 15, 16, 17, 31, 32, 32, 12, 13, 13, 12, 16, 2)])
    none, every = wu.default_cost(12, 0, 0), wu.default_cost(12, 16, 16)
    w_every = expected(mixed, every, 24)
    assert all(d % 12 == 0 for d in w_every[0]["adj_dist"].tolist()) and w_every[1]["edges"] > expected(mixed, none, 24)[1]["edges"]
    out["trim_0_0"], out["trim_16_16"] = (mixed, none, 24, False), (mixed, every, 24, False)
    table = wu.random_cost(5, 7, 1, 2, top=60)
    fam = Nodes([k % 2 for k in range(300)], [code(3 * k) for k in range(300)])
    assert len(set(expected_numpy(fam, table, 60)[0]["adj_dist"].tolist())) > 10
    out["random_table"] = (fam, table, 60, True)
    return out


NAMES = (["no_nodes", "one_node", "equal_R0", "trimmed_only_R0", "conservative_at_cost", "conservative_one_below", "symmetry_3_2", "symmetry_0_0"]
         + [f"tiles_{n}" for n in (255, 256, 257, 513, 1500)] + ["chain"] + [f"class_bits_{k}" for k in range(len(cnu.CLASS_BIT_PAIRS))]
         + ["reach", "cells_255_R65535", "cells_255_one_below", "trim_0_0", "trim_16_16", "random_table"])
_constructed = None


def constructed() -> dict:
    """The lists the host walk and the device are pinned on: name -> (Nodes, cost, R, whether the numpy form serves).  Built
    once."""
    global _constructed
    if _constructed is None:
        out = {}
        out.update(small())
        for ntrim, ctrim in ((3, 2), (0, 0)):
            out[f"symmetry_{ntrim}_{ctrim}"] = symmetry(ntrim, ctrim)[:3] + (False,)
        for n in (255, 256, 257, 513):
            out[f"tiles_{n}"] = tiles(n) + (True,)
        out["tiles_1500"] = tiles(1500, 3) + (True,)      # six blocks
        out.update(components())
        out.update(reach())
        out.update(costs())
        assert sorted(out) == sorted(NAMES)
        _constructed = out
    return _constructed


def wanted(name: str):
    """The contract's (result, stats) of a constructed list: computed once, shared, left unchanged."""
    if name not in _wanted:
        nodes, cost, R, numpy = constructed()[name]
        _wanted[name] = (expected_numpy if numpy else expected)(nodes, cost, R)
    return _wanted[name]


def planted(n: int, n_classes: int, seed: int) -> Nodes:
    """n nodes in n_classes classes: random strings of 11 .. 16 letters, a fifth of them planted near an earlier one (one or two
    substitutions, or a block of one or two letters put in or taken out)."""
    rnd = random.Random(seed)
    strings, classes = [], []
    for k in range(n):
        if k % 5 == 4:
            model = rnd.randrange(len(strings))
            classes.append(classes[model])      # (a planted node shares its model's class)
            s = list(strings[model])
            how = rnd.randrange(4)
            if how < 2:
                for _ in range(how + 1):
                    s[rnd.randrange(len(s))] = rnd.choice(AMINO)
            elif how == 2:
                p = rnd.randrange(len(s) + 1)
                s[p:p] = [rnd.choice(AMINO) for _ in range(rnd.randrange(1, 3))]
            else:
                p = rnd.randrange(len(s) - 2)
                del s[p:p + rnd.randrange(1, 3)]
            strings.append("".join(s))
        else:
            classes.append(rnd.randrange(n_classes))
            strings.append("".join(rnd.choice(AMINO) for _ in range(rnd.randrange(11, 17))))
    return Nodes(classes, strings, [1 + rnd.randrange(50) for _ in range(n)])


# ---- the walk on the host (tests/host_cdr3wnet) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_cdr3wnet")])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        _host.cdr3wnet_host_network.restype = u64
        _host.cdr3wnet_host_network.argtypes = [u64, vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, u64]
    return _host


def host_network(nodes: Nodes, cost, R: int):
    """(degree, adj_off, adj, adj_dist) of the host walk."""
    off, text = cnu.node_text(nodes.strings)
    cls = np.array(nodes.classes, dtype=np.uint32) if len(nodes) else np.zeros(1, np.uint32)
    tt = np.frombuffer(text + b"\0", np.uint8)
    sub = np.ascontiguousarray(cost.sub, dtype=np.uint8)
    m = len(nodes)
    degree, adj_off = np.zeros(max(m, 1), np.uint32), np.zeros(m + 1, np.uint64)
    args = [m, cls.ctypes.data, off.ctypes.data, tt.ctypes.data, sub.ctypes.data, cost.gap, cost.ntrim, cost.ctrim, R]
    one = np.zeros(1, np.uint32)
    need = host_lib().cdr3wnet_host_network(*args, degree.ctypes.data, adj_off.ctypes.data, one.ctypes.data, one.ctypes.data, 0)
    adj, dist = np.zeros(max(need, 1), np.uint32), np.zeros(max(need, 1), np.uint32)
    assert host_lib().cdr3wnet_host_network(*args, degree.ctypes.data, adj_off.ctypes.data, adj.ctypes.data, dist.ctypes.data, need) == need
    return degree[:m], adj_off, adj[:need], dist[:need]
