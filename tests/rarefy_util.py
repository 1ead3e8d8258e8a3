"""What the downsampling tests share (`overlap --downsample`, `overlap --diversity`; include/dcrx.h "downsample"): the contract
as Python that shares no method with the kernels — every key of a sample computed with numpy uint64 arithmetic and sorted, a
count per row; the abundance classes and the diversity table from the raw list of cells with Python integers and Fractions,
never through classes —, the stand-ins for the native calls, the constructed tables with the premise each is for, and the host
build of the shared code and of the primitive's steps (tests/host_rarefy)."""
import ctypes as C
import functools
import math
import os
import subprocess
from collections import Counter
from fractions import Fraction

import numpy as np

from decombinator_amd import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_rarefy", "build", "librarefy_host.so")
MASK = (1 << 64) - 1
SAMPLE_STEP, READ_STEP = 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15
OUTPUTS = ("kept", "reads", "depth_used", "threshold")


class Invalid(Exception):
    """What the contract answers with DCRX_E_INVALID."""


class Unsupported(Exception):
    """What the contract answers with DCRX_E_UNSUPPORTED."""


# ---- the key, in Python integers and in numpy ----

def fin(z: int) -> int:
    z &= MASK
    z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27; z = z * 0x94D049BB133111EB & MASK
    return z ^ z >> 31


def key(seed: int, s: int, r: int) -> int:
    return fin(fin(seed + (s + 1) * SAMPLE_STEP) + (r + 1) * READ_STEP)


@functools.lru_cache(maxsize=8)
def sample_keys(seed: int, s: int, X: int) -> np.ndarray:
    """key(seed, s, r) for r = 0 .. X - 1 (read only: shared between the cases that need it)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.arange(1, X + 1, dtype=np.uint64) * u(READ_STEP) + u(fin(seed + (s + 1) * SAMPLE_STEP))
        z ^= z >> u(30); z *= u(0xBF58476D1CE4E5B9)
        z ^= z >> u(27); z *= u(0x94D049BB133111EB)
        z ^= z >> u(31)
    z.setflags(write=False)
    return z


# ---- the contract ----

def expected_downsample(samples, weights, n_samples, depths, seed) -> dict:
    """The four outputs as nat.downsample gives them: every key, sorted, and a count per row."""
    S, m = int(n_samples), len(samples)
    smp = np.asarray(samples, dtype=np.int64).reshape(-1)
    w = np.asarray(weights, dtype=np.uint64).reshape(-1)
    if S < 1 or (m and (smp.max() >= S or smp.min() < 0 or (np.diff(smp) < 0).any())):
        raise Invalid("samples")
    if m >= 1 << 30 or w.sum(dtype=np.float64) >= 2.0 ** 40:      # (exact below 2^53, and a weight above that is refused anyway)
        raise Unsupported("size")
    kept = np.zeros(m, np.uint64)
    reads, used, thr = [0] * S, [0] * S, [0] * S
    first = np.searchsorted(smp, np.arange(S + 1))      # (the ids are non-decreasing: a sample's rows are first[s] .. first[s + 1])
    for s in range(S):
        ws = w[first[s]:first[s + 1]]
        X = int(ws.sum())
        n = min(int(depths[s]), X)
        reads[s], used[s] = X, n
        if n == X:
            thr[s] = MASK
            kept[first[s]:first[s + 1]] = ws
            continue
        keys = sample_keys(int(seed), s, X)
        thr[s] = int(np.sort(keys)[n])
        below = np.concatenate(([0], np.cumsum(keys < np.uint64(thr[s])))).astype(np.uint64)
        ends = np.cumsum(ws)
        kept[first[s]:first[s + 1]] = below[ends] - below[ends - ws]
    return {"kept": kept, "reads": np.array(reads, np.uint64), "depth_used": np.array(used, np.uint64),
            "threshold": np.array(thr, np.uint64)}


def assert_same(got: dict, want: dict):
    """Every output, exactly."""
    for k in OUTPUTS:
        assert [int(x) for x in got[k]] == [int(x) for x in want[k]], k


def assert_sums(result: dict, samples):
    """What holds for every result: a sample's kept reads add up to depth_used."""
    per = [0] * len(result["reads"])
    for a, k in zip(samples, result["kept"]):
        per[int(a)] += int(k)
    assert per == [int(x) for x in result["depth_used"]]
    assert all(int(u) <= int(x) for u, x in zip(result["depth_used"], result["reads"]))


def cells_of(samples, groups, weights, n_samples) -> list:
    """Per sample the weights of its cells (sample, group) that are not zero — the raw list everything below starts from."""
    S = int(n_samples)
    cells = {}
    for a, g, w in zip(samples, groups, weights):
        a, g, w = int(a), int(g), int(w)
        if not 0 <= a < S:
            raise Invalid("sample")
        cells[(a, g)] = cells.get((a, g), 0) + w
    if any(w >= 1 << 32 for w in cells.values()):
        raise Unsupported("a cell weight")
    return [[w for (a, _g), w in cells.items() if a == s and w] for s in range(S)]


def expected_classes(samples, groups, weights, n_samples) -> dict:
    """The CSR nat.abundance_classes gives."""
    off, count, mult = [0], [], []
    for ws in cells_of(samples, groups, weights, n_samples):
        for c, k in sorted(Counter(ws).items()):
            count.append(c); mult.append(k)
        off.append(len(count))
    return {"class_off": np.array(off, np.uint64), "class_count": np.array(count, np.uint32), "class_mult": np.array(mult, np.uint64)}


def assert_same_classes(got: dict, want: dict):
    for k in ("class_off", "class_count", "class_mult"):
        assert [int(x) for x in got[k]] == [int(x) for x in want[k]], k


def six(x) -> str:
    return format(float(x), ".6f")


def diversity_rows(names, reads_in, cells) -> list:
    """The `overlap_diversity.tsv` fields per sample from the raw cell weights (cells_of), cell by cell."""
    rows = []
    for name, x_in, ws in zip(names, reads_in, cells):
        X, R = sum(ws), len(ws)
        f1, f2 = ws.count(1), ws.count(2)
        d50 = held = 0
        for w in sorted(ws, reverse=True):
            if 2 * held >= X:
                break
            held += w; d50 += 1
        up = sorted(ws)
        shannon = -math.fsum(w / X * math.log(w / X) for w in ws) if X else 0.0
        rows.append([
            name, str(int(x_in)), str(X), str(R), str(f1), str(f2), str(max(ws, default=0)), str(d50),
            six(R + Fraction(f1 * (f1 - 1), 2 * (f2 + 1))),
            six(Fraction(sum(w * (w - 1) for w in ws), X * (X - 1))) if X >= 2 else "nan",
            six(Fraction(X * X, sum(w * w for w in ws))) if X else "nan",
            six(Fraction(sum((2 * i - R - 1) * w for i, w in enumerate(up, 1)), R * X)) if X else "nan",
            six(shannon), six(1 - shannon / math.log(R)) if R >= 2 else "nan"])
    return rows


FLOAT_COLUMNS = ("shannon", "clonality")      # summed in another order on the other side: compared within 2e-6


def assert_diversity(text: bytes, want_rows: list):
    lines = [ln.split("\t") for ln in text.decode().splitlines()]
    assert lines[0] == nat.OVERLAP_DIVERSITY_COLUMNS and len(lines) == len(want_rows) + 1
    for got, want in zip(lines[1:], want_rows):
        for col, g, w in zip(lines[0], got, want):
            if col in FLOAT_COLUMNS and "nan" not in (g, w):
                assert abs(float(g) - float(w)) <= 2e-6, (col, g, w)
            else:
                assert g == w, (col, g, w)


# ---- the stand-ins for the native calls in the CPU tests of the stage ----

def python_downsample(calls=None):
    def downsample(samples, weights, n_samples, depths, seed):
        if calls is not None:
            calls.append(("downsample", np.asarray(samples).tolist(), np.asarray(weights).tolist(), int(n_samples),
                          np.asarray(depths).tolist(), int(seed)))
        return expected_downsample(samples, weights, n_samples, depths, seed)
    return downsample


def python_classes(calls=None):
    def abundance_classes(samples, groups, weights, n_samples):
        if calls is not None:
            calls.append(("abundance_classes", np.asarray(samples).tolist(), np.asarray(groups).tolist(), np.asarray(weights).tolist(),
                          int(n_samples)))
        return expected_classes(samples, groups, weights, n_samples)
    return abundance_classes


# ---- the host build (tests/host_rarefy) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_rarefy")])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        for name in ("tile", "slots", "bins", "grid", "levels", "candidates", "max_samples"):
            getattr(_host, "rarefy_host_" + name).restype = u32
        _host.rarefy_host_fin.restype, _host.rarefy_host_fin.argtypes = u64, [u64]
        _host.rarefy_host_key.restype, _host.rarefy_host_key.argtypes = u64, [u64, u64, u64]
        _host.rarefy_host_digit.restype, _host.rarefy_host_digit.argtypes = u32, [u64, u32]
        _host.rarefy_host_prefix.restype, _host.rarefy_host_prefix.argtypes = u64, [u64, u32]
        _host.rarefy_host_run_kept.restype, _host.rarefy_host_run_kept.argtypes = u32, [u64, u64, u32]
        _host.rarefy_host_downsample.restype = C.c_int
        _host.rarefy_host_downsample.argtypes = [u32, u32, vp, vp, vp, u64, u32, vp, vp, vp, vp, vp]
    return _host


def constant(name: str) -> int:
    """TILE, SLOTS, BINS, GRID, LEVELS, CANDIDATES as the kernels have them."""
    return int(getattr(host_lib(), "rarefy_host_" + name.lower())())


def host_downsample(samples, weights, n_samples, depths, seed, grid):
    """rarefy_host_downsample — the primitive's steps on the host, for `grid` blocks: (the four outputs, the levels per sample)."""
    smp, w, d = np.ascontiguousarray(samples, np.uint32), np.ascontiguousarray(weights, np.uint64), np.ascontiguousarray(depths, np.uint64)
    m, S = len(smp), int(n_samples)
    kept, levels = np.zeros(max(m, 1), np.uint64), np.zeros(S, np.uint32)
    reads, used, thr = (np.zeros(S, np.uint64) for _ in range(3))
    rc = host_lib().rarefy_host_downsample(S, m, smp.ctypes.data, w.ctypes.data, d.ctypes.data, int(seed), int(grid), kept.ctypes.data,
                                           reads.ctypes.data, used.ctypes.data, thr.ctypes.data, levels.ctypes.data)
    assert rc == 0, rc
    return {"kept": kept[:m], "reads": reads, "depth_used": used, "threshold": thr}, [int(x) for x in levels]


# ---- constructed tables: name -> (samples, weights, n_samples, depths, seed), with what each is for.  The edges come from
# the kernels' own constants ----

def _table(parts, depths, seed):
    """parts: (sample, rows, weight) runs in order."""
    samples, weights = [], []
    for s, n, w in parts:
        samples += [s] * n
        weights += [w] * n
    return samples, weights, len(depths), list(depths), seed


def _make_constructed() -> dict:
    TILE, SLOTS = constant("TILE"), constant("SLOTS")
    out = {
        "one_read_depth_0": lambda: _table([(0, 1, 1)], [0], 1),
        "one_read_depth_1": lambda: _table([(0, 1, 1)], [1], 1),
        "empty_sample_between": lambda: _table([(0, 3, 5), (2, 4, 6)], [7, 3, 10], 2),
        "zero_weight_rows": lambda: _table([(0, 2, 0), (0, 3, 4), (0, 3, 0), (0, 2, 9), (0, 2, 0), (1, 1, 0), (1, 4, 3), (1, 1, 0)], [11, 5], 3),
        "depth_0_whole_and_real": lambda: _table([(0, 5, 7), (1, 5, 7), (2, 50, 7)], [0, 35, 100], 4),
        "depth_above_x": lambda: _table([(0, 5, 7), (1, 9, 3)], [36, MASK], 4),
        "heavy_row_between_light": lambda: _table([(0, 1, 1), (0, 1, 3 * TILE + 5), (0, 1, 1)], [TILE], 5),
        "tile_rows_of_weight_1": lambda: _table([(0, TILE, 1), (0, 3, 2)], [TILE // 2], 6),
        "slots_plus_1_rows_of_weight_1": lambda: _table([(0, SLOTS + 1, 1), (0, 1, TILE)], [SLOTS], 6),
        "zero_runs_longer_than_slots": lambda: _table([(0, SLOTS + 3, 0), (0, 2, 10), (0, 2 * SLOTS, 0), (0, 1, 5), (1, SLOTS + 1, 0),
                                                       (1, 60, 1), (1, SLOTS + 1, 0)], [9, 30], 7),
    }
    for d in (-1, 0, 1):
        out[f"row_end_at_tile{d:+d}"] = lambda d=d: _table([(0, 1, TILE + d), (0, 3, 1), (1, 5, 40)], [TILE // 2, 100], 3)
        out[f"sample_end_at_tile{d:+d}"] = lambda d=d: _table([(0, 10, 10), (0, 1, TILE + d - 100), (2, 50, 3)], [TILE // 3, 7, 60], 4)
    return out


_constructed = None


def constructed_names() -> list:
    global _constructed
    if _constructed is None:
        _constructed = _make_constructed()
    return list(_constructed)


@functools.lru_cache(maxsize=None)
def constructed(name: str):
    """(table, expected_downsample(table)) of a constructed table: made once and shared; nobody changes it."""
    constructed_names()
    table = _constructed[name]()
    return table, expected_downsample(*table)


def premise(name: str, table, want):
    """What a constructed table is for, asserted on the table and the Python reference, never on a device result."""
    samples, weights, S, depths, _ = table
    TILE, SLOTS = constant("TILE"), constant("SLOTS")
    ends = np.cumsum(weights)
    if name.startswith("row_end_at_tile"):
        assert int(ends[0]) == TILE + int(name[-2:]) and weights[1] == 1
    elif name.startswith("sample_end_at_tile"):
        last = max(i for i, a in enumerate(samples) if a == 0)
        assert int(ends[last]) == TILE + int(name[-2:]) and samples[last + 1] == 2      # ... and sample 1 has no rows
    elif name == "heavy_row_between_light":
        assert weights == [1, 3 * TILE + 5, 1] and 0 < int(want["kept"][1]) < weights[1]
    elif name == "tile_rows_of_weight_1":
        assert weights[:TILE] == [1] * TILE and SLOTS < TILE      # the rows behind the first SLOTS are looked up in the offsets
    elif name == "slots_plus_1_rows_of_weight_1":
        assert weights[:SLOTS + 1] == [1] * (SLOTS + 1) and SLOTS + 1 < TILE
    elif name == "zero_runs_longer_than_slots":
        assert weights[:SLOTS + 3] == [0] * (SLOTS + 3) and sum(weights) < TILE
    elif name == "depth_0_whole_and_real":
        assert [int(x) for x in want["depth_used"]] == [0, 35, 100] and int(want["threshold"][1]) == MASK
    elif name == "empty_sample_between":
        assert 1 not in samples and int(want["reads"][1]) == 0 and int(want["threshold"][1]) == MASK
    if name not in ("one_read_depth_1", "depth_above_x"):
        assert any(0 < int(u) < int(x) for u, x in zip(want["depth_used"], want["reads"])) or name == "one_read_depth_0"


def skew_table():
    """One sample: 10^5 rows of weights 1 .. 40 around one row that holds 15 % of the reads (about 2.4 million in all)."""
    small = [1 + k % 40 for k in range(100000)]
    heavy = sum(small) * 15 // 85
    weights = small[:50000] + [heavy] + small[50000:]
    return [0] * len(weights), weights


def second_tile_table():
    """The smallest total at which blocks take a second tile: GRID tiles and one read, in rows of 1 .. 4096 reads."""
    total = constant("GRID") * constant("TILE") + 1
    weights, k = [], 0
    while sum(weights) < total:
        weights.append(min(1 + (k * 2654435761) % 4096, total - sum(weights)) if k % 7 else 0)
        k += 1
    return [0] * len(weights), weights


def many_samples_table():
    """64 samples of unequal size — 50 + 997 s reads — in rows of 1 .. 9 reads, and depths around them."""
    samples, weights, depths = [], [], []
    for s in range(64):
        left, k = 50 + 997 * s, 0
        while left:
            w = min(left, 1 + (k * 7 + s) % 9)
            samples.append(s); weights.append(w)
            left -= w; k += 1
        depths.append((50 + 997 * s) * (s % 5) // 4 if s % 7 else 20000)
    return samples, weights, depths
