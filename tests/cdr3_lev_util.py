"""What the tests of the CDR3 network's Levenshtein metric share (`--cdr3-network --cdr3-metric levenshtein`, include/dcrx.h
"the CDR3 network's metric"): the contract as plain Python that shares no method with the kernels (candidate pairs by hashing
every string with up to D characters deleted — symmetric deletion —, each confirmed by a plain DP; components by a union-find
that keeps the smallest rank), the stand-in for _native.cdr3_network that knows `metric`, the edge file's text with the DP
distance, a generator of families with indels, and the host build of the pair test (tests/host_cdr3lev)."""
import ctypes as C
import itertools
import os
import random

import numpy as np

from decombinator_amd import _native as nat
from tests import cdr3_network_util as cnu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_cdr3lev", "build", "libcdr3lev_host.so")
MAX_LEN = cnu.MAX_LEN


# ---- the contract ----

def lev(a: bytes, b: bytes) -> int:
    """The Levenshtein distance by the plain table (substitution, insertion and deletion cost 1 each), over what is left of
    the two strings once their common prefix and suffix are set aside (those never take part in a cheapest script)."""
    p = 0
    while p < len(a) and p < len(b) and a[p] == b[p]:
        p += 1
    a, b = a[p:], b[p:]
    q = 0
    while q < len(a) and q < len(b) and a[-1 - q] == b[-1 - q]:
        q += 1
    a, b = a[:len(a) - q], b[:len(b) - q]
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def _deletions(s: bytes, D: int) -> set:
    """s with 0 .. D characters deleted: two strings within D edits share one of these (each edit script of e <= D edits is
    undone on either side by deleting at most e characters)."""
    out = front = {s}
    for _ in range(D):
        front = {t[:p] + t[p + 1:] for t in front for p in range(len(t))}
        out = out | front
    return out


def _pairs(members, strings, D):
    """Per member of one class the set of its neighbours: candidates share a deletion variant, the DP confirms."""
    near = {i: set() for i in members}
    seen = {}
    for i in members:
        for v in _deletions(strings[i], D):
            seen.setdefault(v, []).append(i)
    checked = {}
    for group in seen.values():
        if len(group) < 2:
            continue
        distinct = {}
        for i in group:
            distinct.setdefault(strings[i], []).append(i)
        keys = list(distinct)
        for x in range(len(keys)):
            for y in range(x, len(keys)):
                a, b = keys[x], keys[y]
                k = (a, b) if a <= b else (b, a)
                if k not in checked:
                    checked[k] = abs(len(a) - len(b)) <= D and lev(a, b) <= D
                if checked[k]:
                    for i in distinct[a]:
                        near[i].update(distinct[b])
                    for j in distinct[b]:
                        near[j].update(distinct[a])
    for i in members:
        near[i].discard(i)
    return near


def expected_lev_network(classes, strings, weights, D):
    """(result, stats) as nat.cdr3_network(..., metric="levenshtein") gives them with want_edges, from the contract; the shape
    of cnu.expected_network."""
    assert D in (1, 2)
    strings = cnu.as_bytes(strings)
    m = len(strings)
    buckets = {}
    out_of_reach = 0
    for i, s in enumerate(strings):
        if 1 <= len(s) <= MAX_LEN:
            buckets.setdefault(int(classes[i]), []).append(i)
        else:
            out_of_reach += 1
    near = {}
    for members in buckets.values():
        near.update(_pairs(members, strings, D))
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, ns in near.items():
        for j in ns:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)      # the root is the smallest rank
    root = [find(i) for i in range(m)]
    heads = sorted(set(root))
    row = {h: r for r, h in enumerate(heads)}
    size, weight = [0] * len(heads), [0] * len(heads)
    for i in range(m):
        size[row[root[i]]] += 1
        weight[row[root[i]]] += int(weights[i])
    degree = [len(near.get(i, ())) for i in range(m)]
    adj_off = np.zeros(m + 1, dtype=np.uint64)
    if m:
        adj_off[1:] = np.cumsum(degree)
    adj = [j for i in range(m) for j in sorted(near.get(i, ()))]
    result = {"degree": np.array(degree, dtype=np.uint32), "cluster_of": np.array([row[r] for r in root], dtype=np.uint32),
              "cluster_head": np.array(heads, dtype=np.uint32), "cluster_size": np.array(size, dtype=np.uint32),
              "cluster_weight": np.array(weight, dtype=np.uint64), "adj_off": adj_off, "adj": np.array(adj, dtype=np.uint32)}
    stats = {"nodes_in": m, "out_of_reach": out_of_reach, "edges": len(adj) // 2, "clusters_out": len(heads),
             "singletons": sum(1 for x in size if x == 1), "largest_cluster": max(size, default=0), "largest_degree": max(degree, default=0)}
    assert list(stats) == list(nat.CDR3_NETWORK_STATS)
    return result, stats


def edge_kinds(strings, result, D):
    """(edges between two lengths, edges of one length that the Hamming metric misses at D: more than D substitutions apart)
    of a result with edges."""
    strings = cnu.as_bytes(strings)
    off, adj = result["adj_off"], result["adj"]
    two_lengths = not_hamming = 0
    for a in range(len(strings)):
        for b in adj[int(off[a]):int(off[a + 1])].tolist():
            if a < b:
                if len(strings[a]) != len(strings[b]):
                    two_lengths += 1
                elif sum(x != y for x, y in zip(strings[a], strings[b])) > D:
                    not_hamming += 1
    return two_lengths, not_hamming


def brute_force_native(calls=None):
    """What stands in for _native.cdr3_network in the CPU tests of the stage: cnu's for hamming, the contract above for
    levenshtein, in the native function's shape.  calls: a list that receives every call's (classes, strings, distance,
    want_edges, the keywords the caller named)."""
    def cdr3_network(classes, aa_off, aa_text, weights, distance, want_edges=False, **more):
        assert set(more) <= {"metric"}, more
        strings = cnu.node_strings(aa_off, aa_text)
        if calls is not None:
            calls.append((np.asarray(classes).tolist(), strings, int(distance), bool(want_edges), dict(more)))
        metric = more.get("metric", "hamming")
        assert metric in ("hamming", "levenshtein"), metric
        expected = cnu.expected_network if metric == "hamming" else expected_lev_network
        result, stats = expected(classes, strings, weights, distance)
        if not want_edges:
            del result["adj_off"], result["adj"]
        return result, stats
    return cdr3_network


def edges_text(strings, result) -> str:
    """The `.cdr3_edges.tsv` text under the Levenshtein metric: every edge a < b, ascending by (a, b), with the DP distance."""
    strings = cnu.as_bytes(strings)
    lines = ["\t".join(nat.CDR3_EDGE_COLUMNS)]
    off, adj = result["adj_off"], result["adj"]
    for a in range(len(strings)):
        for b in adj[int(off[a]):int(off[a + 1])].tolist():
            if a < b:
                lines.append(f"{a}\t{b}\t{lev(strings[a], strings[b])}")
    return "\n".join(lines) + "\n"


# ---- generators ----

def edit(s: str, k: int, rnd) -> str:
    """s after k edits, each a substitution, an insertion or a deletion with equal chance (a string of one letter is not
    emptied, one of MAX_LEN letters does not grow)."""
    t = list(s)
    for _ in range(k):
        kind = rnd.randrange(3)
        if kind == 1 and len(t) >= MAX_LEN:
            kind = 0
        if kind == 2 and len(t) <= 1:
            kind = 0
        if kind == 0:
            p = rnd.randrange(len(t))
            t[p] = rnd.choice([c for c in cnu.AMINO if c != t[p]])
        elif kind == 1:
            t.insert(rnd.randrange(len(t) + 1), rnd.choice(cnu.AMINO))
        else:
            del t[rnd.randrange(len(t))]
    return "".join(t)


def families_indel(n: int, seed: int, length: int = 20) -> list:
    """As cnu.families — seeds of `length` random letters, each followed by a family of 3 to 10 strings 1 to 3 edits from it,
    three in five of them one —, but each edit is a substitution, an insertion or a deletion with equal chance."""
    rnd = random.Random(seed)
    out = []
    while len(out) < n:
        s = "".join(rnd.choice(cnu.AMINO) for _ in range(length))
        out.append(s)
        for _ in range(rnd.randrange(3, 11)):
            out.append(edit(s, rnd.choice((1, 1, 1, 2, 3)), rnd))
    rnd.shuffle(out)
    return out[:n]


# ---- the pair test on the host (tests/host_cdr3lev) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_cdr3lev")])
        _host = C.CDLL(HOST_LIB)
        _host.cdr3lev_host_pack.restype, _host.cdr3lev_host_pack.argtypes = None, [C.c_char_p, C.c_uint64, C.c_void_p]
        _host.cdr3lev_host_lev_within.restype = C.c_uint32
        _host.cdr3lev_host_lev_within.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        _host.cdr3lev_host_lev_within_many.restype = None
        _host.cdr3lev_host_lev_within_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        _host.cdr3lev_host_presence.restype, _host.cdr3lev_host_presence.argtypes = C.c_uint32, [C.c_void_p, C.c_uint32]
        _host.cdr3lev_host_presence_allows.restype = C.c_int
        _host.cdr3lev_host_presence_allows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        _host.cdr3lev_host_key_class.restype, _host.cdr3lev_host_key_class.argtypes = C.c_uint64, [C.c_uint64]
        _host.cdr3lev_host_key_length.restype, _host.cdr3lev_host_key_length.argtypes = C.c_uint32, [C.c_uint64]
    return _host


def host_pack(s: bytes) -> np.ndarray:
    """A string of 0 .. 32 bytes as the kernels hold it: eight words, zero beyond the length."""
    out = np.full(8, 0xFFFFFFFF, dtype=np.uint32)
    host_lib().cdr3lev_host_pack(s, len(s), out.ctypes.data)
    return out


def host_lev_within(a: bytes, b: bytes, D: int) -> int:
    pa, pb = host_pack(a), host_pack(b)
    return int(host_lib().cdr3lev_host_lev_within(pa.ctypes.data, len(a), pb.ctypes.data, len(b), D))


def host_lev_within_many(pairs, D: int) -> np.ndarray:
    """lev_within of every (a, b) of `pairs` in one call."""
    flat = [s for p in pairs for s in p]
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        off[1:] = np.cumsum([len(s) for s in flat])
    text = np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8)
    out = np.zeros(max(1, len(pairs)), dtype=np.uint32)
    host_lib().cdr3lev_host_lev_within_many(text.ctypes.data, off.ctypes.data, len(pairs), D, out.ctypes.data)
    return out[:len(pairs)]


def host_presence(s: bytes) -> int:
    return int(host_lib().cdr3lev_host_presence(host_pack(s).ctypes.data, len(s)))
