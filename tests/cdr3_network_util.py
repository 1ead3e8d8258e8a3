"""What the CDR3 network tests share (`--clonotypes --cdr3-network`, include/dcrx.h "the CDR3 network"): the contract as plain
Python that shares no method with the kernels (pairs by hashing strings with one or two positions masked out, components by a
union-find that keeps the smallest rank), the stand-in for _native.cdr3_network, the files' texts from the column lists,
generators, and the host build of the per-node and per-pair code (tests/host_cdr3net)."""
import ctypes as C
import os
import random

import numpy as np

from decombinator_amd import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_cdr3net", "build", "libcdr3net_host.so")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
MAX_LEN = 32


# ---- nodes ----

def as_bytes(strings) -> list:
    return [s if isinstance(s, bytes) else str(s).encode("latin-1") for s in strings]


def node_text(strings):
    """(aa_off, aa_text) of a list of strings."""
    bs = as_bytes(strings)
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return off, b"".join(bs)


def node_strings(aa_off, aa_text) -> list:
    return [bytes(aa_text[int(aa_off[k]):int(aa_off[k + 1])]) for k in range(len(aa_off) - 1)]


# ---- the contract ----

def _pairs(members, strings, D):
    """Per member of one bucket (equal class, equal length) the set of its neighbours: two strings within D substitutions agree
    once the (at most D) positions at which they differ are masked out."""
    near = {i: set() for i in members}
    L = len(strings[members[0]])
    masks = [(p,) for p in range(L)]
    if D == 2:
        masks += [(p, q) for p in range(L) for q in range(p + 1, L)]
    for mask in masks:
        seen = {}
        for i in members:
            s = bytearray(strings[i])
            for p in mask:
                s[p] = 0
            seen.setdefault(bytes(s), []).append(i)      # (the masked positions are the same for the whole table: 0 stands for "any")
        for group in seen.values():
            if len(group) > 1:
                for i in group:
                    near[i].update(group)
    for i in members:
        near[i].discard(i)
    return near


def expected_network(classes, strings, weights, D):
    """(result, stats) as nat.cdr3_network gives them with want_edges, from the contract."""
    assert D in (1, 2)
    strings = as_bytes(strings)
    m = len(strings)
    buckets = {}
    out_of_reach = 0
    for i, s in enumerate(strings):
        if 1 <= len(s) <= MAX_LEN:
            buckets.setdefault((int(classes[i]), len(s)), []).append(i)
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


def brute_force_native(calls=None):
    """What stands in for _native.cdr3_network in the CPU tests of the stage: the contract above, in the native function's
    shape.  calls: a list that receives every call's (classes, strings, distance, want_edges)."""
    def cdr3_network(classes, aa_off, aa_text, weights, distance, want_edges=False):
        strings = node_strings(aa_off, aa_text)
        if calls is not None:
            calls.append((np.asarray(classes).tolist(), strings, int(distance), bool(want_edges)))
        result, stats = expected_network(classes, strings, weights, distance)
        if not want_edges:
            del result["adj_off"], result["adj"]
        return result, stats
    return cdr3_network


def assert_same(got, want):
    """(result, stats) of nat.cdr3_network against expected_network: the statistics and every array, exactly; the CSR where the
    result has it."""
    (gr, gs), (wr, ws) = got, want
    assert gs == ws, (gs, ws)
    for k in ("degree", "cluster_of", "cluster_head", "cluster_size", "cluster_weight"):
        assert np.array_equal(np.asarray(gr[k], dtype=np.uint64), np.asarray(wr[k], dtype=np.uint64)), k
    if "adj_off" in gr:
        assert np.array_equal(np.asarray(gr["adj_off"], dtype=np.uint64), wr["adj_off"]), "adj_off"
        assert np.array_equal(np.asarray(gr["adj"], dtype=np.uint32), wr["adj"]), "adj"


# ---- the files, from the column lists ----

def file_text(v_calls, j_calls, strings, weights, result) -> str:
    """The `.cdr3_clusters.tsv` text: per node its v_call, j_call, string and weight, and what `result` says of it."""
    strings = as_bytes(strings)
    lines = ["\t".join(nat.CDR3_CLUSTER_COLUMNS)]
    for i, s in enumerate(strings):
        c = int(result["cluster_of"][i])
        lines.append("\t".join([str(i), v_calls[i], j_calls[i], s.decode("latin-1"), str(int(weights[i])), str(c),
                                str(int(result["cluster_size"][c])), str(int(result["cluster_weight"][c])), str(int(result["degree"][i]))]))
    return "\n".join(lines) + "\n"


def edges_text(strings, result) -> str:
    """The `.cdr3_edges.tsv` text: every edge a < b, ascending by (a, b), with the distance of the two strings."""
    strings = as_bytes(strings)
    lines = ["\t".join(nat.CDR3_EDGE_COLUMNS)]
    off, adj = result["adj_off"], result["adj"]
    for a in range(len(strings)):
        for b in adj[int(off[a]):int(off[a + 1])].tolist():
            if a < b:
                lines.append(f"{a}\t{b}\t{sum(x != y for x, y in zip(strings[a], strings[b]))}")
    return "\n".join(lines) + "\n"


def call_classes(v_calls, j_calls, mode: str) -> list:
    """The classes of nodes with these calls under --cdr3-class `mode`, numbered by first appearance (only which nodes share
    a class enters the contract)."""
    seen = {}
    key = {"none": lambda v, j: (), "v": lambda v, j: (v,), "vj": lambda v, j: (v, j)}[mode]
    return [seen.setdefault(key(v, j), len(seen)) for v, j in zip(v_calls, j_calls)]


def same_partition(a, b) -> bool:
    """Whether two class lists put the same nodes together."""
    fwd, back = {}, {}
    return len(a) == len(b) and all(fwd.setdefault(x, y) == y and back.setdefault(y, x) == x for x, y in zip(a, b))


# ---- generators ----

def mutate(s: str, k: int, rnd) -> str:
    """s with k positions substituted (each by another letter)."""
    t = list(s)
    for p in rnd.sample(range(len(t)), k):
        t[p] = rnd.choice([c for c in AMINO if c != t[p]])
    return "".join(t)


def families(n: int, seed: int, length: int = 20) -> list:
    """n strings: seeds of `length` random letters, each followed by a family of 3 to 10 strings that differ from it in 1 to 3
    places, three in five of them in one (purely random strings have almost no neighbours and would test nothing)."""
    rnd = random.Random(seed)
    out = []
    while len(out) < n:
        s = "".join(rnd.choice(AMINO) for _ in range(length))
        out.append(s)
        for _ in range(rnd.randrange(3, 11)):
            out.append(mutate(s, rnd.choice((1, 1, 1, 2, 3)), rnd))
    rnd.shuffle(out)
    return out[:n]


def path(k: int, seed: int = 1):
    """k <= 200 strings of length 12 in which string t + 1 changes position t mod 12 of string t to a letter that position has
    not held: consecutive strings are at distance 1, all others at >= 2.  The ranks are shuffled: returns (strings in rank
    order, the rank of path position t)."""
    assert 1 <= k <= 200
    cur, chain = ["A"] * 12, []
    used = [1] * 12
    for t in range(k):
        chain.append("".join(cur))
        cur[t % 12] = AMINO[used[t % 12]]
        used[t % 12] += 1
    rank = list(range(k))
    random.Random(seed).shuffle(rank)
    out = [None] * k
    for t, r in enumerate(rank):
        out[r] = chain[t]
    return out, rank


def star(k: int, length: int = 20, centre_rank=None):
    """A centre and k - 1 leaves, each one substitution from it: leaf t changes position t mod length (leaves that change one
    position are neighbours of each other too; up to `length` leaves it is a star proper).  The centre takes `centre_rank`
    (default: the last)."""
    assert 1 <= k - 1 <= length * (len(AMINO) - 1)
    centre = "A" * length
    leaves = [centre[:t % length] + AMINO[1 + t // length] + centre[t % length + 1:] for t in range(k - 1)]
    at = k - 1 if centre_rank is None else centre_rank
    return leaves[:at] + [centre] + leaves[at:]


# ---- decoys of the walk: strings whose packed words are equal, classes that differ in their high bits ----

ZERO_RUN = (b"CASSF", b"CASSF\x00", b"CASSF\x00\x00")
ZERO_RUN_FRONT = 254          # nodes of a smaller class in front: the run's buckets then straddle sorted position 256


def zero_byte_run(front_strings):
    """(classes, strings, the rank of ZERO_RUN[0]): the front strings under class 0, then under class 1 a run of strings that a
    zero byte lengthens — the packed words are equal, the lengths are not —, a pair of 31 and 32 bytes of the same kind, and one
    substitution of the run's head.  By (class, length) the run stands at sorted positions 254 (with its substitution at 255),
    256 and 257; by class alone, in rank order, at 254, 255 and 256."""
    assert len(front_strings) == ZERO_RUN_FRONT
    long = bytes(range(65, 65 + 31))
    tail = list(ZERO_RUN) + [long, long + b"\x00", b"CASSY"]
    packed = [host_pack(x).tolist() for x in tail]
    assert packed[0] == packed[1] == packed[2] and packed[3] == packed[4] and [len(x) for x in tail] == [5, 6, 7, 31, 32, 5]
    return [0] * ZERO_RUN_FRONT + [1] * len(tail), as_bytes(front_strings) + tail, ZERO_RUN_FRONT


CLASS_BIT_PAIRS = ((0, 1 << 31), (5, 5 | 1 << 26), (0xFFFFFFFE, 0xFFFFFFFF))


def class_bit_nodes(strings, pair, n_out=0, seed=3):
    """(classes, strings, the same classes as 0 and 1): every string once under either class of `pair`, ranks shuffled, with n_out
    nodes out of reach (under the pair's larger class) among them.  The strings of one class are those of the other: across the
    classes every node has a twin at distance 0."""
    rnd = random.Random(seed)
    nodes = [(c, s) for s in as_bytes(strings) for c in (0, 1)] + [(1, b"" if k % 2 else b"A" * (MAX_LEN + 1)) for k in range(n_out)]
    rnd.shuffle(nodes)
    return [pair[c] for c, _ in nodes], [s for _, s in nodes], [c for c, _ in nodes]


def no_edge_across(classes, result) -> bool:
    off, adj = result["adj_off"], result["adj"]
    return all(classes[a] == classes[int(b)] for a in range(len(classes)) for b in adj[int(off[a]):int(off[a + 1])])


# ---- the per-node and per-pair code on the host (tests/host_cdr3net) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_cdr3net")])
        _host = C.CDLL(HOST_LIB)
        for name in ("words", "max_len", "key_bits"):
            getattr(_host, "cdr3net_host_" + name).restype = C.c_uint32
        _host.cdr3net_host_key_out_of_reach.restype = C.c_uint64
        _host.cdr3net_host_in_reach.restype, _host.cdr3net_host_in_reach.argtypes = C.c_int, [C.c_uint64]
        _host.cdr3net_host_key.restype, _host.cdr3net_host_key.argtypes = C.c_uint64, [C.c_uint32, C.c_uint64]
        _host.cdr3net_host_pack.restype, _host.cdr3net_host_pack.argtypes = None, [C.c_char_p, C.c_uint64, C.c_void_p]
        _host.cdr3net_host_distance.restype, _host.cdr3net_host_distance.argtypes = C.c_uint32, [C.c_void_p, C.c_void_p, C.c_uint32]
    return _host


def host_pack(s: bytes) -> np.ndarray:
    out = np.full(8, 0xFFFFFFFF, dtype=np.uint32)
    host_lib().cdr3net_host_pack(s, len(s), out.ctypes.data)
    return out
