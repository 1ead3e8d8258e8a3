"""What the overlap tests share (the `overlap` sub-command, include/dcrx.h "overlap"): the contract as plain Python that shares
no method with the kernels (a dict keyed by (class, bytes) to per-sample sums, plain loops for the planes, Python integers,
`sorted` with a tuple key: no hashing scheme, no sorting network, no rounds), the stand-in for _native.overlap, the files'
texts, generators, the constructed cells and tables that pin the pair kernel and the host entry with the premise each is
for, and the host build of the per-row and per-pair code and of the pair kernel's walk (tests/host_overlap)."""
import ctypes as C
import functools
import os
import random

import numpy as np

from decombinator_amd import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_overlap", "build", "liboverlap_host.so")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
LIMIT = 1 << 32


class Unsupported(Exception):
    """What the contract answers with DCRX_E_UNSUPPORTED."""


def as_bytes(strings) -> list:
    return [s if isinstance(s, bytes) else str(s).encode("latin-1") for s in strings]


def row_text(strings):
    """(off, text) of a list of strings."""
    bs = as_bytes(strings)
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return off, b"".join(bs)


def row_strings(off, text) -> list:
    return [bytes(text[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)]


# ---- the contract ----

def expected_overlap(samples, classes, strings, weights, n_samples, min_samples=2):
    """(result, stats) as nat.overlap gives them, from the contract."""
    S = int(n_samples)
    strings = as_bytes(strings)
    m = len(strings)
    assert 1 <= S <= 64 and min_samples >= 1 and len(samples) == len(classes) == len(weights) == m
    cells, heads = {}, {}      # key -> {sample: sum}; key -> first rank (dicts keep the order of first appearance)
    per_sample = [0] * S
    for i in range(m):
        a, w = int(samples[i]), int(weights[i])
        assert 0 <= a < S
        if w >= LIMIT:
            raise Unsupported("a row weight")
        key = (int(classes[i]), strings[i])
        heads.setdefault(key, i)
        per = cells.setdefault(key, {})
        per[a] = per.get(a, 0) + w
        per_sample[a] += 1
    keys = list(cells)                      # first appearance = head ascending
    number = {key: g for g, key in enumerate(keys)}
    if any(w >= LIMIT for per in cells.values() for w in per.values()):
        raise Unsupported("a cell weight")
    planes = {name: [[0] * S for _ in range(S)] for name in nat.OVERLAP_PLANES}
    for per in cells.values():
        for a, wa in per.items():
            for b, wb in per.items():
                planes["shared"][a][b] += 1
                planes["shared_weight"][a][b] += wa
                planes["min_weight"][a][b] += min(wa, wb)
                planes["prod_lo"][a][b] += (wa * wb) % LIMIT
                planes["prod_hi"][a][b] += (wa * wb) >> 32
    public = [key for key in keys if len(cells[key]) >= min_samples]
    public = sorted(public, key=lambda key: (-len(cells[key]), -sum(cells[key].values()), heads[key]))
    cell_off, cell_sample, cell_weight = [0], [], []
    for key in public:
        for a in sorted(cells[key]):
            cell_sample.append(a)
            cell_weight.append(cells[key][a])
        cell_off.append(len(cell_sample))
    result = {name: np.array(planes[name], dtype=object).reshape(S, S) for name in nat.OVERLAP_PLANES}
    result.update(group_of=np.array([number[(int(classes[i]), strings[i])] for i in range(m)], dtype=np.uint32),
                  head=np.array([heads[k] for k in public], dtype=np.uint32),
                  n_samples=np.array([len(cells[k]) for k in public], dtype=np.uint32),
                  weight=np.array([sum(cells[k].values()) for k in public], dtype=np.uint64),
                  cell_off=np.array(cell_off, dtype=np.uint64), cell_sample=np.array(cell_sample, dtype=np.uint32),
                  cell_weight=np.array(cell_weight, dtype=np.uint64))
    sizes = [len(per) for per in cells.values()]
    stats = {"rows_in": m, "groups": len(keys), "private_groups": sum(1 for x in sizes if x == 1),
             "shared_groups": sum(1 for x in sizes if x >= 2), "in_all_samples": sum(1 for x in sizes if x == S),
             "largest_n_samples": max(sizes, default=0), "public_rows": len(public), "public_cells": len(cell_sample)}
    assert list(stats) == list(nat.OVERLAP_STATS)
    stats["rows_per_sample"] = per_sample
    return result, stats


def brute_force_native(calls=None):
    """What stands in for _native.overlap in the CPU tests of the stage: the contract above, in the native function's shape.
    calls: a list that receives every call's (samples, classes, strings, weights, n_samples, min_samples)."""
    def overlap(samples, classes, off, text, weights, n_samples, min_samples=2):
        strings = row_strings(off, text)
        if calls is not None:
            calls.append((np.asarray(samples).tolist(), np.asarray(classes).tolist(), strings, np.asarray(weights).tolist(),
                          int(n_samples), int(min_samples)))
        return expected_overlap(samples, classes, strings, weights, n_samples, min_samples)
    return overlap


def _ints(a) -> list:
    return [int(x) for x in np.asarray(a, dtype=object).reshape(-1)]


def assert_invariants(result, stats, weights):
    """What holds for every result (the issue's invariants)."""
    S = len(result["shared"])
    sh, mw, sw = (np.asarray(result[k], dtype=object) for k in ("shared", "min_weight", "shared_weight"))
    assert int(result["cell_off"][-1]) == len(result["cell_sample"]) == sum(_ints(result["n_samples"])) == stats["public_cells"]
    for a in range(S):
        for b in range(S):
            assert int(sh[a][b]) == int(sh[b][a]) and int(mw[a][b]) == int(mw[b][a])
            assert int(sh[a][b]) <= min(int(sh[a][a]), int(sh[b][b]))
    assert sum(int(sw[a][a]) for a in range(S)) == sum(int(w) for w in weights)
    if stats["public_rows"] == stats["groups"]:      # (min_samples = 1: every group is a row, and its n_samples is there)
        assert sum(_ints(result["n_samples"])) == sum(int(sh[a][a]) for a in range(S))


def assert_same(got, want, weights=None):
    """(result, stats) of nat.overlap against expected_overlap: the statistics and every array, exactly."""
    (gr, gs), (wr, ws) = got, want
    assert gs == ws, (gs, ws)
    for k in nat.OVERLAP_PLANES:
        assert _ints(gr[k]) == _ints(wr[k]), k
    for k in ("group_of", "head", "n_samples", "weight", "cell_off", "cell_sample", "cell_weight"):
        assert _ints(gr[k]) == _ints(wr[k]), k
    if weights is not None:
        assert_invariants(gr, gs, weights)
        assert_invariants(wr, ws, weights)


# ---- the files ----

def clonotypes_text(rows) -> bytes:
    """A `.clonotypes.tsv` from (v_call, j_call, junction_aa, duplicate_count) rows; the other columns are filled in."""
    lines = ["\t".join(nat.CLONOTYPE_COLUMNS)]
    for v, j, aa, dup in rows:
        lines.append("\t".join([v, j, aa, str(dup), "1", "TGT" * len(aa), "0, 0, 0, 0, ", str(dup)]))
    return ("\n".join(lines) + "\n").encode("latin-1")


def public_text(result, names, v_calls, j_calls, strings) -> bytes:
    """The `overlap_public.tsv` text from a result and the rows' columns, formatted in Python."""
    strings = as_bytes(strings)
    lines = ["\t".join(nat.OVERLAP_PUBLIC_COLUMNS + list(names)).encode("latin-1")]
    off = _ints(result["cell_off"])
    for r, h in enumerate(_ints(result["head"])):
        per = dict(zip(_ints(result["cell_sample"])[off[r]:off[r + 1]], _ints(result["cell_weight"])[off[r]:off[r + 1]]))
        fields = [v_calls[h].encode("latin-1"), j_calls[h].encode("latin-1"), strings[h], str(int(result["n_samples"][r])).encode(),
                  str(int(result["weight"][r])).encode()] + [str(per.get(a, 0)).encode() for a in range(len(names))]
        lines.append(b"\t".join(fields))
    return b"\n".join(lines) + b"\n"


def call_classes(v_calls, j_calls, mode: str) -> list:
    """The classes of rows with these calls under --overlap-key `mode`, numbered by first appearance."""
    seen = {}
    key = {"none": lambda v, j: (), "v": lambda v, j: (v,), "vj": lambda v, j: (v, j)}[mode]
    return [seen.setdefault(key(v, j), len(seen)) for v, j in zip(v_calls, j_calls)]


# ---- generators ----

def random_tables(n_samples: int, rows: int, pool: int, seed: int):
    """n_samples x rows rows drawn from a pool of (v_call, j_call, string) keys — five V calls, three J calls, strings of 8 to
    16 letters of which some repeat under other calls — with Zipf-like weights: (samples, v_calls, j_calls, strings,
    weights)."""
    rnd = random.Random(seed)
    texts = ["".join(rnd.choice(AMINO) for _ in range(rnd.randrange(8, 17))) for _ in range(pool * 2 // 3)]
    keys = [(f"TRBV{rnd.randrange(5)}", f"TRBJ{rnd.randrange(3)}", rnd.choice(texts)) for _ in range(pool)]
    samples, v, j, s, w = [], [], [], [], []
    for a in range(n_samples):
        for _ in range(rows):
            k = keys[min(pool - 1, int(rnd.paretovariate(0.8)) - 1 if rnd.random() < 0.5 else rnd.randrange(pool))]
            samples.append(a); v.append(k[0]); j.append(k[1]); s.append(k[2])
            w.append(min(1 << 20, int(rnd.paretovariate(1.0))))
    return samples, v, j, s, w


def cells_of_groups(groups):
    """Crafted cells for the pairs primitive: groups = a list of {sample: weight} -> (cell_off, cell_sample, cell_weight) as
    uint32 arrays, samples ascending inside a group."""
    off, smp, wt = [0], [], []
    for per in groups:
        for a in sorted(per):
            smp.append(a); wt.append(per[a])
        off.append(len(smp))
    return np.array(off, dtype=np.uint32), np.array(smp, dtype=np.uint32), np.array(wt, dtype=np.uint32)


def expected_planes(groups, S: int, start=None):
    """The five planes of crafted cells as (5, S, S) Python integers, added onto `start`."""
    P = [[[0] * S for _ in range(S)] for _ in nat.OVERLAP_PLANES] if start is None else [[list(r) for r in p] for p in start]
    for per in groups:
        for a, wa in per.items():
            for b, wb in per.items():
                P[0][a][b] += 1
                P[1][a][b] += wa
                P[2][a][b] += min(wa, wb)
                P[3][a][b] += (wa * wb) % LIMIT
                P[4][a][b] += (wa * wb) >> 32
    return P


# ---- constructed cells for the pair kernel (tests/test_gpu_overlap.py on the device, tests/test_overlap.py through the
# host walk): every list is a list of {sample: weight} ----

PAIR_BLOCK = 256      # the kernel's tile: BLOCK cells, one lane each (dcrx_group.h)
PAIR_GRID = 2048      # ... and the most blocks of a launch (dcrx_overlap.hip); a block takes every gridDim-th tile
PLANE_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
TOP = LIMIT - 1


def pairs_smax(S: int) -> int:
    """The SMAX run_pairs picks for S samples."""
    return next(x for x in (8, 16, 32, 64) if S <= x)


def pairs_grid(n_groups: int, S: int) -> int:
    """The grid launch_pairs picks."""
    return min(PAIR_GRID, max(1, -(-n_groups * S // PAIR_BLOCK)))


def n_cells(groups) -> int:
    return sum(len(per) for per in groups)


def group_starts(groups) -> list:
    """The offset of every group's first cell."""
    out, at = [], 0
    for per in groups:
        out.append(at)
        at += len(per)
    return out


def plane_size_groups(S: int) -> list:
    """Every pair of samples meets, with weights that tell (a, b) from (b, a); the last sample, S - 1, is in a pair with
    every other one and alone in the last group."""
    if S == 1:
        return [{0: 1 + (5 * k) % 97} for k in range(40)] + [{0: 5}]
    groups = [{a: 1 + (3 * a + 5 * k) % 97 for a in range(S) if (a + k) % 3 or a == S - 1} for k in range(40)]
    groups += [{a: 7 + a, S - 1: 9} for a in range(S - 1)]
    return groups + [{S - 1: 5}]


def several_tiles_groups() -> list:
    """S = 3: groups of 1, 2 and 3 cells in turn, until the cells fill more than PAIR_GRID + 1 tiles and 300 cells."""
    groups, cells = [], 0
    while cells <= (PAIR_GRID + 1) * PAIR_BLOCK + 300:
        g = len(groups)
        groups.append({a: 1 + (7 * g + a) % 1000 for a in range(1 + g % 3)})
        cells += 1 + g % 3
    return groups


_TAIL3 = [{1: 4}, {0: 2, 2: 9}, {}, {0: 1, 1: 2, 2: 3}, {2: 8}]


def lookup_groups(empties: int, front: int = 0) -> list:
    """S = 3: `front` single-cell groups, a group of two cells, `empties` empty groups, a group of three cells, a tail.  With
    front a multiple of PAIR_BLOCK the group of two opens a tile, and the end of the group of three is staged end number
    empties + 1: the last staged one at 254 empties, not staged from 255 on."""
    tail = [{k % 3: 20 + k} for k in range(5)]      # (single cells: behind the empties only the group of three needs its end)
    return [{k % 3: 1 + k % 7} for k in range(front)] + [{0: 3, 2: 5}] + [{}] * empties + [{0: 11, 1: 13, 2: 17}] + tail


def lookup_lists() -> dict:
    """name -> (groups, the index of the group whose end is looked up behind the empties or None, its staged slot or None)."""
    out = {}
    for front in (0, 2 * PAIR_BLOCK):
        for e in (253, 254, 255, 256):
            out[f"front{front}_empties{e}"] = (lookup_groups(e, front), front + 1 + e, e + 1)
    body = [{k % 3: 2 + k % 5} for k in range(40)] + _TAIL3
    out["leading_empties"] = ([{}] * 300 + body, None, None)
    out["trailing_empties"] = (body + [{}] * 300, None, None)
    out["full_tile_of_singles"] = ([{k % 3: 1 + k % 9} for k in range(PAIR_BLOCK)] + [{0: 7, 1: 8, 2: 9}] + _TAIL3, None, None)
    return out


def full_group(r: int) -> dict:
    return {a: 1 + (7 * a + 3 * r) % 61 for a in range(64)}


def tile_edge_groups(front: int) -> list:
    """S = 64: `front` single-cell groups, then a group of 64 cells, then a tail."""
    return [{k % 64: 1 + k % 9} for k in range(front)] + [full_group(front)] + [{5: 2}, {0: 1, 63: 4}]


def tile_edge_long_groups() -> list:
    """S = 64: runs of r % 37 single cells, each followed by a group of 64 cells, r = 1 .. 160."""
    groups = []
    for r in range(1, 161):
        groups += [{(r + k) % 64: 1 + (r * k) % 11} for k in range(r % 37)] + [full_group(r)]
    return groups


def straddling_offsets(groups) -> list:
    """Where in its tile every group of 64 cells starts that reaches into the next tile."""
    return [at % PAIR_BLOCK for at, per in zip(group_starts(groups), groups) if len(per) == 64 and at % PAIR_BLOCK + 64 > PAIR_BLOCK]


def limit_weight_groups() -> list:
    """S = 64: three groups of 64 cells with every weight 2^32 - 1, beside 200 groups of small weights."""
    small = [{(3 * k + a * a) % 64: 1 + (k + a) % 29 for a in range(1 + k % 4)} for k in range(200)]
    return small[:100] + [{a: TOP for a in range(64)}] * 2 + small[100:] + [{a: TOP for a in range(64)}]


def one_entry_groups() -> list:
    """S = 1: 200 000 single-cell groups, weights over the whole 32 bits."""
    return [{0: 1 + (k * 2654435761) % TOP} for k in range(200000)]


# What each list is for, asserted on the list and on the Python reference (want = expected_planes), never on a device result:
# a degenerate list cannot pass for a result.

def premise_plane_size(groups, S, want):
    assert all(want[p][a][b] for p in range(4) for a in range(S) for b in range(S))      # no entry that a lost term leaves right
    if S >= 2:
        assert sum(want[1][a][b] == want[1][b][a] for a in range(S) for b in range(a)) <= 2      # shared_weight is not symmetric
        assert any(want[1][a][b] != want[1][b][a] for a in range(S) for b in range(a))
        assert any(0 in per and S - 1 in per for per in groups) and any(S - 2 in per and S - 1 in per for per in groups)
    if S == 64:
        assert len({want[2][a][b] for a in range(S) for b in range(S)}) >= 760


def premise_several_tiles(groups, S, want):
    cells = n_cells(groups)
    assert -(-cells // PAIR_BLOCK) > PAIR_GRID and len(groups) * S >= PAIR_GRID * PAIR_BLOCK      # a saturated grid ...
    assert -(-cells // PAIR_BLOCK) - PAIR_GRID == 3 and cells % PAIR_BLOCK      # ... whose blocks 0, 1, 2 take a second tile, the last one partly filled
    assert {len(per) for per in groups} == {1, 2, 3}


def premise_lookup(name, groups):
    cells, starts = n_cells(groups), group_starts(groups)
    _, g, slot = lookup_lists()[name]
    if g is not None:      # the group of three behind the empties: in the tile its predecessor of two cells opens
        front = g - slot
        assert front % PAIR_BLOCK == 0 and starts[front] == front and len(groups[front]) == 2 and len(groups[g]) == 3
        assert all(not per for per in groups[front + 1:g]) and starts[g] // PAIR_BLOCK == front // PAIR_BLOCK
        assert all(len(per) == 1 for per in groups[g + 1:])      # ... and the only group behind the empties with cells to walk
        assert (slot <= PAIR_BLOCK - 1) == (name.endswith("253") or name.endswith("254"))      # staged, the last slot at 254
        assert (slot == PAIR_BLOCK - 1) == name.endswith("254")
        assert (front > 0) == (front // PAIR_BLOCK == 2)
    elif name == "leading_empties":
        assert all(not per for per in groups[:300]) and groups[300]
    elif name == "trailing_empties":
        assert all(not per for per in groups[-300:]) and groups[-301] and cells % PAIR_BLOCK
    else:
        assert all(len(per) == 1 for per in groups[:PAIR_BLOCK]) and len(groups[PAIR_BLOCK]) == 3 and starts[PAIR_BLOCK] == PAIR_BLOCK


def premise_tile_edge(front, groups):
    at = group_starts(groups)[front]
    assert len(groups[front]) == 64 and at == front and straddling_offsets(groups) == [front]
    assert at + 64 > PAIR_BLOCK and (front != 193 or at + 63 == PAIR_BLOCK)      # 193: one cell in the next tile; 255: 63 cells


def premise_tile_edge_long(groups):
    offs = straddling_offsets(groups)
    assert sum(len(per) == 64 for per in groups) == 160 and len(set(offs)) >= 30 and min(offs) == 193


def premise_limit_weights(groups, want):
    assert sum(1 for per in groups if len(per) == 64 and set(per.values()) == {TOP}) == 3 and len(groups) == 203
    assert all(want[p][a][b] > 1 << 33 for p in (2, 4) for a in range(64) for b in range(64))


def premise_one_entry(groups, want):
    n = len(groups)
    assert n == 200000 and -(-n // PAIR_BLOCK) == 782 == pairs_grid(n, 1)
    ws = [per[0] for per in groups]
    assert [want[p][0][0] for p in range(5)] == [n, sum(ws), sum(ws), sum(w * w % LIMIT for w in ws), sum(w * w >> 32 for w in ws)]
    assert want[4][0][0] > LIMIT


LOOKUP_NAMES = tuple(lookup_lists())
TILE_EDGE_FRONTS = (193, 224, 255)
CONSTRUCTED = {f"plane_size_{S}": (lambda S=S: plane_size_groups(S), S) for S in PLANE_SIZES}      # name -> (the list's maker, S)
CONSTRUCTED["several_tiles"] = (several_tiles_groups, 3)
CONSTRUCTED.update({"lookup_" + k: (lambda k=k: lookup_lists()[k][0], 3) for k in LOOKUP_NAMES})
CONSTRUCTED.update({f"tile_edge_{f}": (lambda f=f: tile_edge_groups(f), 64) for f in TILE_EDGE_FRONTS})
CONSTRUCTED["tile_edge_long"] = (tile_edge_long_groups, 64)
CONSTRUCTED["limit_weights"] = (limit_weight_groups, 64)
CONSTRUCTED["one_entry"] = (one_entry_groups, 1)


@functools.lru_cache(maxsize=None)
def constructed(name: str):
    """(groups, S, expected_planes(groups, S)) of a constructed list: made once and shared; nobody changes it."""
    make, S = CONSTRUCTED[name]
    groups = make()
    return groups, S, expected_planes(groups, S)


# ---- constructed tables for the host entry: (samples, classes, strings, weights) ----

def _keys_of(n: int, stem: str, classes: int) -> list:
    assert n <= 8000
    return [(k % classes, stem + AMINO[k % 20] + AMINO[k // 20 % 20] + AMINO[k // 400]) for k in range(n)]


def _columns(rows):
    return [r[1] for r in rows], [r[0][0] for r in rows], [r[0][1] for r in rows], [r[2] for r in rows]


def block_edge_table(m: int):
    """m rows of about m / 3 keys in S = 3 samples, every weight 3, ranks shuffled; the key of rank 0 has a row again at the
    last rank of the shuffled rows, and an odd m ends with the one row of a key of its own."""
    rnd = random.Random(m)
    n = m - m % 2
    keys = _keys_of(m // 3, "CASS", 2)
    rows = [(key, rnd.randrange(3), 3) for key in keys] + [(rnd.choice(keys), rnd.randrange(3), 3) for _ in range(n - len(keys))]
    rnd.shuffle(rows)
    rows[n - 1] = (rows[0][0], (rows[0][1] + 1) % 3, 3)
    if m % 2:
        rows.append(((0, "CAWWF"), 1, 3))
    return _columns(rows)


def premise_block_edge(m, table, want):
    samples, classes, strings, _ = table
    res, st = want
    g, n = [int(x) for x in res["group_of"]], m - m % 2
    assert len(g) == m and st["public_rows"] == st["groups"] and abs(st["groups"] - m // 3) <= 2
    # a group with its head in the first block and a member in the last block the shuffled rows reach
    assert g[0] == g[n - 1] == 0 and (m < 512 or (n - 1) // 256 == 1)
    if m % 2:      # rank m - 1 is the head of a private group: above one block, alone in its block
        assert g.count(g[m - 1]) == 1 and g[m - 1] == st["groups"] - 1 and (m < 256 or (m - 1) % 256 == 0)
    cells = {}
    for a, gg in zip(samples, g):
        cells[(gg, a)] = cells.get((gg, a), 0) + 1
    per_group = [sum(1 for (gg, _a) in cells if gg == k) for k in range(st["groups"])]
    assert max(cells.values()) >= 2 and set(per_group) == {1, 2, 3}      # repeats inside a sample; one to three samples


def hash_bits_table():
    """6 000 rows drawn from 2 000 keys in 4 samples: at 3 hash bits eight runs of hundreds of keys each."""
    rnd = random.Random(33)
    keys = _keys_of(2000, "CAS", 3)
    rows = [(rnd.choice(keys), rnd.randrange(4), 1 + k % 17) for k in range(6000)]
    return _columns(rows)


def long_cell_table(extra: int = 0):
    """One key with 1 000 rows of sample 0 whose weights add up to 2^32 - 1 + extra (and a row in samples 1 and 2), beside
    600 rows of 600 other keys, ranks shuffled."""
    rnd = random.Random(44)
    big = (0, "CASSLONGF")
    rows = [(big, 0, 4294967)] * 999 + [(big, 0, 4294967 + 295 + extra), (big, 1, 5), (big, 2, 7)]
    rows += [(key, rnd.randrange(3), 1 + k % 50) for k, key in enumerate(_keys_of(600, "CASR", 2))]
    rnd.shuffle(rows)
    return _columns(rows)


def premise_long_cell(table, want):
    samples, classes, strings, weights = table
    res, _ = want
    g = [int(x) for x in res["group_of"]]
    big = [k for k in range(len(g)) if strings[k] == "CASSLONGF" and samples[k] == 0]
    assert len(big) == 1000 and sum(weights[k] for k in big) == TOP and len({g[k] for k in big}) == 1
    first = sum(1 for k in range(len(g)) if (g[k], samples[k]) < (g[big[0]], 0))      # where the cell sort puts the cell's rows
    assert (first + 999) // 256 - first // 256 == 3      # four blocks
    row = [int(x) for x in res["head"]].index(min(big + [k for k in range(len(g)) if strings[k] == "CASSLONGF"]))
    at = int(res["cell_off"][row])
    assert int(res["cell_sample"][at]) == 0 and int(res["cell_weight"][at]) == TOP


# ---- the per-row and per-pair code on the host (tests/host_overlap) ----

_host = None


def host_pairs(groups, S: int, smax: int, grid: int, start=None):
    """overlap_host_pairs — the pair kernel's walk on the host — over crafted cells: the (5, S, S) planes as Python integers."""
    off, smp, wt = cells_of_groups(groups)
    planes = np.zeros(5 * S * S, np.uint64) if start is None else np.array(start, dtype=np.uint64).reshape(-1).copy()
    rc = host_lib().overlap_host_pairs(len(groups), off.ctypes.data, smp.ctypes.data, wt.ctypes.data, S, smax, grid, planes.ctypes.data)
    assert rc == 0, rc
    return [[[int(x) for x in r] for r in p] for p in planes.reshape(5, S, S)]


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_overlap")])
        _host = C.CDLL(HOST_LIB)
        u32, u64, cp = C.c_uint32, C.c_uint64, C.c_char_p
        for name in ("max_samples", "sample_bits", "planes"):
            getattr(_host, "overlap_host_" + name).restype = u32
        _host.overlap_host_hash.restype, _host.overlap_host_hash.argtypes = u64, [u32, cp, u64]
        _host.overlap_host_equal.restype, _host.overlap_host_equal.argtypes = C.c_int, [u32, cp, u64, u32, cp, u64]
        _host.overlap_host_product.restype, _host.overlap_host_product.argtypes = None, [u64, u64, C.POINTER(u64), C.POINTER(u64)]
        _host.overlap_host_full_index.restype, _host.overlap_host_full_index.argtypes = u32, [u32, u32, u32]
        _host.overlap_host_tri_index.restype, _host.overlap_host_tri_index.argtypes = u32, [u32, u32]
        _host.overlap_host_tri_size.restype, _host.overlap_host_tri_size.argtypes = u32, [u32]
        _host.overlap_host_cell_key.restype, _host.overlap_host_cell_key.argtypes = u64, [u32, u32]
        _host.overlap_host_pairs.restype = C.c_int
        _host.overlap_host_pairs.argtypes = [u32, C.c_void_p, C.c_void_p, C.c_void_p, u32, u32, u32, C.c_void_p]
    return _host
