"""What the motif-group tests share (`motifs --groups`; include/dcrx.h "motif groups"): the contract as plain Python that shares
no method with the kernels — the members of a motif from the set of a unit's slices, the global edges from a comparison of
every pair of units, the groups from a union-find kept in a dict, numbered by their smallest unit —, the stand-in for the
native call, the selection rule and the two files' texts written a second time, and the host build of the shared header's new
code (tests/host_motif_groups)."""
import os
import subprocess
from fractions import Fraction

import numpy as np

from tests import motif_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_motif_groups")
UNIT_FIELDS = ("group_of", "n_motifs", "degree")
GROUP_FIELDS = ("head", "units", "weight")


class Invalid(Exception):
    """What the contract answers with DCRX_E_INVALID."""


def motif_number(k: int, code: int) -> int:
    return {2: 0, 3: 26 ** 2, 4: 26 ** 2 + 26 ** 3}[k] + code


def letters_of(k: int, code: int) -> bytes:
    return bytes(65 + code // 26 ** (k - 1 - i) % 26 for i in range(k))


def check_selected(selected, ks):
    """selected: a list of (k, code).  Strictly ascending motif order, every k in K, every code below 26^k."""
    last = -1
    for k, code in selected:
        if k not in ks or k not in (2, 3, 4) or not 0 <= code < 26 ** k:
            raise Invalid(f"({k}, {code}) is no motif of K")
        if motif_number(k, code) <= last:
            raise Invalid(f"({k}, {code}) is out of order")
        last = motif_number(k, code)


def linked(a: bytes, b: bytes, G: int) -> bool:
    """Two units (at two indices) under Hamming at distance G, every class equal: 1 .. 32 bytes, one length, at most G
    positions differ."""
    return G > 0 and 1 <= len(a) <= 32 and len(a) == len(b) and sum(x != y for x, y in zip(a, b)) <= G


def expected_members(units, ks, trim, selected, cap=None) -> dict:
    """What the members primitive gives: n_motifs per unit, mem_off, mem (the rows laid end to end, below cap), need."""
    ks = sorted(set(int(k) for k in ks))
    check_selected(selected, ks)
    sets = [mu.motif_set(u, ks, trim) if mu.takes_part(u) else set() for u in units]
    rows = [[i for i, held in enumerate(sets) if (k, letters_of(k, code)) in held] for k, code in selected]
    mem = [i for row in rows for i in row]
    n_motifs = [0] * len(units)
    for i in mem:
        n_motifs[i] += 1
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    return {"n_motifs": np.array(n_motifs, np.uint32), "mem_off": off, "need": len(mem),
            "mem": np.array(mem if cap is None else mem[:int(cap)], np.uint32), "rows": rows}


def components(n: int, pairs) -> list:
    """group_of per unit from the linked pairs: a union-find in a dict, groups numbered by their smallest unit."""
    parent = {}

    def find(x):
        while parent.get(x, x) != x:
            parent[x] = parent.get(parent[x], parent[x])
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = [find(i) for i in range(n)]
    smallest = {}
    for i, r in enumerate(roots):
        smallest.setdefault(r, i)
    number = {r: g for g, r in enumerate(sorted(smallest, key=smallest.get))}
    return [number[r] for r in roots]


def motifs_held(units, ks, trim, at_least=2) -> list:
    """The motifs at least `at_least` of the units hold, in motif order, as (k, code)."""
    count = {}
    for u in units:
        if mu.takes_part(u):
            for mo in mu.motif_set(u, ks, trim):
                count[mo] = count.get(mo, 0) + 1
    return sorted(((k, mu.code_of(w)) for (k, w), c in count.items() if c >= at_least), key=lambda kc: motif_number(*kc))


def groups_table(n: int, rows, ring=True) -> tuple:
    """A table for the groups primitive on n units: the weights i * i + 1, an adjacency that is no Hamming one (every seventh unit
    linked to the next seventh; none without `ring`) beside the member rows `rows`, and what the contract gives for them through
    components(): (weights, adjacency, {"group_of", "head", "units", "weight"} as lists)."""
    seventh = list(range(0, n, 7)) if ring else []
    adjacency = [[] for _ in range(n)]
    for a, b in zip(seventh, seventh[1:]):
        adjacency[a].append(b)
        adjacency[b].append(a)
    adjacency = [sorted(x) for x in adjacency]
    weights = [i * i + 1 for i in range(n)]
    pairs = [(a, b) for a in range(n) for b in adjacency[a]] + [(row[0], x) for row in rows for x in row[1:]]
    group_of = components(n, pairs)
    g = max(group_of) + 1 if n else 0
    want = {"group_of": group_of, "head": [group_of.index(r) for r in range(g)], "units": [group_of.count(r) for r in range(g)],
            "weight": [sum(w for w, r2 in zip(weights, group_of) if r2 == r) for r in range(g)]}
    return weights, adjacency, want


def csr(lists, dtype=np.uint32) -> tuple:
    """(offsets, entries) of a list of lists."""
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    return off, np.array([x for row in lists for x in row], dtype)


def expected_groups(units, weights, ks=(2, 3, 4), trim=(3, 3), selected=(), G=1, mem_cap=None) -> dict:
    """What nat.cdr3_motif_groups gives for the units (a list of bytes, taken as given), their weights, the selected motifs (a
    list of (k, code) in motif order) and the global distance G."""
    units = [bytes(u) for u in units]
    n = len(units)
    if G not in (0, 1, 2) or max(trim) > 16 or min(trim) < 0:
        raise Invalid("settings")
    members = expected_members(units, ks, trim, list(selected))
    edges = [(a, b) for a in range(n) for b in range(a + 1, n) if linked(units[a], units[b], G)]
    degree = [0] * n
    for a, b in edges:
        degree[a] += 1
        degree[b] += 1
    row_links = [(row[0], other) for row in members["rows"] for other in row[1:]]
    group_of = components(n, edges + row_links)
    groups = max(group_of) + 1 if n else 0
    head, size, weight = [None] * groups, [0] * groups, [0] * groups
    for i, g in enumerate(group_of):
        if head[g] is None:
            head[g] = i
        size[g] += 1
        weight[g] = (weight[g] + int(weights[i])) % (1 << 64)
    with_edge = {group_of[a] for a, _ in edges}
    with_row = {group_of[row[0]] for row in members["rows"] if len(row) >= 2}
    need = members["need"]
    fits = mem_cap is None or need <= int(mem_cap)
    return {"group_of": np.array(group_of, np.uint32), "n_motifs": members["n_motifs"], "degree": np.array(degree, np.uint32),
            "head": np.array(head, np.uint32), "units": np.array(size, np.uint32), "weight": np.array(weight, np.uint64),
            "mem_off": members["mem_off"], "mem": members["mem"] if fits else members["mem"][:0], "need": need,
            "stats": {"units": n, "take_part": sum(mu.takes_part(u) for u in units), "selected": len(selected), "member_pairs": need,
                      "global_edges": len(edges), "groups": groups, "singleton_groups": sum(s == 1 for s in size),
                      "largest_group": max(size, default=0), "mixed_groups": len(with_edge & with_row)}}


def assert_same(got: dict, want: dict):
    """Every field, `need` and the statistics (but the number of rounds, which is the kernels' own), exactly."""
    for f in UNIT_FIELDS + GROUP_FIELDS + ("mem_off", "mem"):
        assert [int(x) for x in got[f]] == [int(x) for x in want[f]], f
    assert int(got["need"]) == int(want["need"])
    assert {k: v for k, v in got["stats"].items() if k != "rounds"} == {k: v for k, v in want["stats"].items() if k != "rounds"}


def assert_same_members(got: dict, want: dict):
    for f in ("n_motifs", "mem_off", "mem"):
        assert [int(x) for x in got[f]] == [int(x) for x in want[f]], f
    assert int(got["need"]) == int(want["need"])


def cut(off, text) -> list:
    return [bytes(text[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def native_stand_in(off, text, weights, ks, trim, sel_k, sel_code, distance=1, mem_cap=None) -> dict:
    """nat.cdr3_motif_groups' signature over the contract (for the stage tests, which run without a GPU)."""
    out = expected_groups(cut(off, text), weights, ks, trim, list(zip((int(k) for k in sel_k), (int(c) for c in sel_code))), distance, mem_cap)
    out["stats"]["rounds"] = 0
    return out


# ---- the selection rule and the files, written a second time

def selected_rows(result: dict, resamples: int, p_text: str, fold_text: str) -> list:
    """The rows of a motifs result that are selected: (ge + 1) / (R + 1) <= p and cs R >= fold sum."""
    p, fold, R = Fraction(p_text), Fraction(fold_text), int(resamples)
    return [r for r in range(len(result["k"]))
            if Fraction(int(result["ge"][r]) + 1, R + 1) <= p and int(result["cs"][r]) * R >= fold * int(result["sum"][r])]


def groups_lines(units, rows_of_unit, reads_of_unit, want: dict, selected) -> list:
    """The `.cdr3_groups.tsv` lines (without the header) from a contract result."""
    held = [[] for _ in units]
    off = [int(x) for x in want["mem_off"]]
    for s, (k, code) in enumerate(selected):
        for i in want["mem"][off[s]:off[s + 1]]:
            held[int(i)].append(letters_of(k, code).decode())
    out = []
    for i, u in enumerate(units):
        g = int(want["group_of"][i])
        out.append("\t".join([u.decode("latin-1"), str(rows_of_unit[i]), str(reads_of_unit[i]), str(g), str(int(want["units"][g])),
                              str(int(want["weight"][g])), str(int(want["degree"][i])), ",".join(held[i]) or "."]))
    return out


def member_lines(units, want: dict, selected, trim) -> list:
    """The `.cdr3_motif_members.tsv` lines (without the header): (motif order, unit order); the first window that holds it."""
    off = [int(x) for x in want["mem_off"]]
    out = []
    for s, (k, code) in enumerate(selected):
        letters = letters_of(k, code)
        for i in want["mem"][off[s]:off[s + 1]]:
            u = units[int(i)]
            at = min(p for p in range(trim[0], len(u) - trim[1] - k + 1) if u[p:p + k] == letters)
            out.append("\t".join([letters.decode(), str(k), u.decode("latin-1"), str(at), str(int(want["group_of"][int(i)]))]))
    return out


# ---- the host build of the shared header's new code

def host_program(target: str = "all") -> str:
    subprocess.check_call(["make", "-s", "-C", HOST_DIR, target])
    return os.path.join(HOST_DIR, "build", "motif_groups_asan" if target == "asan" else "motif_groups_host")
