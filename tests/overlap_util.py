"""What the overlap tests share (the `overlap` sub-command, include/dcrx.h "overlap"): the contract as plain Python that shares
no method with the kernels (a dict keyed by (class, bytes) to per-sample sums, plain loops for the planes, Python integers,
`sorted` with a tuple key: no hashing scheme, no sorting network, no rounds), the stand-in for _native.overlap, the files'
texts, generators, and the host build of the per-row and per-pair code (tests/host_overlap)."""
import ctypes as C
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


# ---- the per-row and per-pair code on the host (tests/host_overlap) ----

_host = None


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
    return _host
