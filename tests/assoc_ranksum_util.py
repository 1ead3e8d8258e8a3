"""What the rank-sum association tests share (`associate --test rank-sum`; include/dcrx.h "association, rank-sum"): the contract
as Python that shares no method with the kernels — a feature's scores decoded from its planes, a rank sum as a matrix product of
0/1 labels and scores, the cell of a score by numpy's searchsorted —, the doubled mid-ranks by brute force and the per-feature
integers in Python integers, the constructed cases, the stand-in for the native call, the stage's files from their definitions
and the host build of the shared code and of the primitive's steps (tests/host_assoc_ranksum)."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction
from math import isqrt, sqrt

import numpy as np

from tests import assoc_util as au
from tests.assoc_util import Invalid, Unsupported

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_assoc_ranksum")
HOST_LIB = os.path.join(HOST_DIR, "build", "libassoc_ranksum_host.so")
HOST_MAIN = os.path.join(HOST_DIR, "build", "assoc_ranksum_main")
OUTPUTS = ("obs_score", "labels", "perm_max", "exceed", "tail")
STATS = ("features", "features_weighted", "weight", "permutations", "tail_total", "max_perm_score")
ALTERNATIVES = ("greater", "less", "two-sided")
PLANES, SHIFT, MAX_EDGES = 7, 20, 1024
MAX_SAMPLES, MAX_PERMUTATIONS, MAX_FEATURES, MAX_WEIGHT = 64, 1 << 20, 1 << 30, 1 << 32
U32 = (1 << 32) - 1


# ---- the statistic, by brute force and in Python integers ----

def mid_rank_scores(x, depths=None) -> list:
    """a[s] of one feature from its values x[s] (already cut at --min-count): the doubled mid-rank less its minimum; with depths
    the order is that of x[s] / depths[s], by cross-multiplication."""
    n = len(x)
    if depths is None:
        depths = [1] * n

    def less(s, t):
        return x[s] * depths[t] < x[t] * depths[s]

    def same(s, t):
        return x[s] * depths[t] == x[t] * depths[s]
    d = [2 * sum(less(t, s) for t in range(n)) + sum(same(t, s) for t in range(n)) + 1 for s in range(n)]
    return [v - min(d) for v in d]


def sums(a, n1: int):
    """(A, B, Q, offset, scale) of one feature's scores."""
    N, A, B = len(a), sum(a), sum(v * v for v in a)
    Q = N * B - A * A
    return A, B, Q, n1 * A, (min(U32, isqrt((1 << 64) // Q)) if Q else 0)


def planes_of(a) -> list:
    return [sum(((v >> b) & 1) << s for s, v in enumerate(a)) for b in range(PLANES)]


def inputs_of(scores, n1: int):
    """(planes [F, 7] uint64, offsets, scales uint32) of a list of per-feature score lists."""
    F = len(scores)
    planes = np.array([planes_of(a) for a in scores], dtype=np.uint64).reshape(F, PLANES)
    off = np.array([sums(a, n1)[3] for a in scores], dtype=np.uint32)
    sc = np.array([sums(a, n1)[4] for a in scores], dtype=np.uint32)
    return planes, off, sc


def score(D: int, scale: int, alternative: int) -> int:
    u = D if alternative == 0 else -D if alternative == 1 else abs(D)
    return (min(max(u, 0), (1 << SHIFT) - 1) * scale) >> SHIFT


def z_of(D: int, Q: int, N: int, n1: int) -> float:
    return D * sqrt((N - 1) / (n1 * (N - n1) * Q))


# ---- the contract ----

def refuse(N, C_, alternative, F, E, P):
    """The scalars, in the header's order."""
    if not 2 <= N <= MAX_SAMPLES:
        raise Invalid("samples")
    if C_ >> N or C_ == 0 or C_ == (1 << N) - 1:
        raise Invalid("case mask")
    if alternative > 2:
        raise Invalid("alternative")
    if E > MAX_EDGES:
        raise Invalid("edges")
    if F >= MAX_FEATURES or P > MAX_PERMUTATIONS:
        raise Unsupported("size")


def expected_ranksum(planes, offsets, scales, mults, n_samples, case_mask, alternative, edges, permutations, seed, clean=False) -> dict:
    """The contract of dcrx_assoc_ranksum (clean: the device entry's — planes are cut to N bits and nothing of the arrays is
    refused)."""
    N, C_, P = int(n_samples), int(case_mask), int(permutations)
    alt = ALTERNATIVES.index(alternative) if isinstance(alternative, str) else int(alternative)
    planes = np.asarray(planes, dtype=np.uint64).reshape(-1, PLANES)
    off, sc = np.asarray(offsets, dtype=np.int64), np.asarray(scales, dtype=np.int64)
    mults, edges = np.asarray(mults, dtype=np.uint64), np.asarray(edges, dtype=np.int64)
    F, E = len(planes), len(edges)
    refuse(N, C_, alt, F, E, P)
    n1 = bin(C_).count("1")
    bits = np.uint64((1 << N) - 1)
    if clean:
        planes = planes & bits
    else:
        if F and int((planes & ~bits).max()):
            raise Invalid("a plane with a bit at or above N")
        if E > 1 and not (edges[1:] > edges[:-1]).all():
            raise Invalid("edges not strictly ascending")
        if int(mults.sum(dtype=object) if F else 0) >= MAX_WEIGHT:
            raise Unsupported("multiplicity sum")
    at = np.arange(N, dtype=np.uint64)
    a = np.zeros((F, N), dtype=np.int64)      # the scores, decoded
    for b in range(PLANES):
        a += (((planes[:, b, None] >> at[None, :]) & np.uint64(1)).astype(np.int64)) << b

    def t_of(label_bits):      # [n, N] 0/1 -> [n, F]
        D = N * (label_bits @ a.T) - off[None, :]
        u = D if alt == 0 else -D if alt == 1 else np.abs(D)
        return (np.clip(u, 0, (1 << SHIFT) - 1) * sc[None, :]) >> SHIFT
    cases = np.array([[(C_ >> s) & 1 for s in range(N)]], dtype=np.int64)
    obs = t_of(cases)[0] if F else np.zeros(0, np.int64)
    L = au.labels_numpy(seed, P, N, n1)
    most, exceed, tail = np.zeros(P, dtype=np.int64), np.zeros(F, dtype=np.int64), np.zeros(E, dtype=np.uint64)
    part = mults > 0
    lo, hi = (mults & np.uint64(0xFFFF)).astype(np.float64), (mults >> np.uint64(16)).astype(np.float64)      # exact in float64 sums
    if F and P:
        for p0 in range(0, P, 256):
            Lb = ((L[p0:p0 + 256, None] >> at[None, :]) & np.uint64(1)).astype(np.int64)
            t = t_of(Lb)
            exceed += (t >= obs[None, :]).sum(axis=0)
            if part.any():
                most[p0:p0 + 256] = t[:, part].max(axis=1)
            if E:
                j = np.searchsorted(edges, t, side="right") - 1
                inside = (j >= 0) & part[None, :]
                if inside.any():
                    jj = j[inside]
                    tail += (np.bincount(jj, np.broadcast_to(lo, t.shape)[inside], E).astype(np.uint64)
                             + (np.bincount(jj, np.broadcast_to(hi, t.shape)[inside], E).astype(np.uint64) << np.uint64(16)))
    stats = {"features": F, "features_weighted": int(part.sum()), "weight": int(mults.sum(dtype=object)) if F else 0, "permutations": P,
             "tail_total": int(tail.sum(dtype=object)) if E else 0, "max_perm_score": int(most.max()) if P else 0}
    return {"obs_score": obs.astype(np.uint32), "labels": L, "perm_max": most.astype(np.uint32), "exceed": exceed.astype(np.uint32), "tail": tail,
            "stats": stats}


def enumerated(scores, offsets, scales, mults, N, C_, alt, edges, P, seed) -> dict:
    """The contract once more for small N, pair by pair in Python integers over the relabelings the contract draws (au.labels)."""
    n1 = bin(C_).count("1")
    F = len(scores)

    def t(f, Lmask):
        W = sum(v for s, v in enumerate(scores[f]) if Lmask >> s & 1)
        return score(N * W - int(offsets[f]), int(scales[f]), alt)
    obs = [t(f, C_) for f in range(F)]
    exceed, most, tail = [0] * F, [0] * P, [0] * len(edges)
    for p in range(P):
        Lmask = au.labels(seed, p, N, n1)
        for f in range(F):
            v = t(f, Lmask)
            exceed[f] += v >= obs[f]
            if not mults[f]:
                continue
            most[p] = max(most[p], v)
            below = [j for j, e in enumerate(edges) if e <= v]
            if below:
                tail[below[-1]] += int(mults[f])
    return {"obs_score": obs, "perm_max": most, "exceed": exceed, "tail": tail}


def assert_same(got: dict, want: dict, what=""):
    for key in OUTPUTS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        assert np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, key, np.flatnonzero(g.astype(np.uint64) != w.astype(np.uint64))[:8])


def python_ranksum(calls=None):
    """The stand-in for nat.assoc_ranksum: the contract, with a record of the calls."""
    def run(*args):
        if calls is not None:
            calls.append(args)
        return expected_ranksum(*args)
    return run


# ---- the host build (tests/host_assoc_ranksum) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", HOST_DIR])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        for name in ("lanes", "perms_per_lane", "block_perms", "slice", "group", "planes", "shift", "max_edges"):
            getattr(_host, "assoc_ranksum_host_" + name).restype = u32
        _host.assoc_ranksum_host_weighted_sum.restype, _host.assoc_ranksum_host_weighted_sum.argtypes = u32, [vp, u64]
        _host.assoc_ranksum_host_score_of.restype, _host.assoc_ranksum_host_score_of.argtypes = u32, [u32, u32, u32, u32, u32]
        _host.assoc_ranksum_host_edge_of.restype, _host.assoc_ranksum_host_edge_of.argtypes = u32, [vp, u32, u32]
        _host.assoc_ranksum_host_refuse.restype, _host.assoc_ranksum_host_refuse.argtypes = C.c_int, [u32, u64, u32, u64, u32, u32]
        _host.assoc_ranksum_host_run.restype = C.c_int
        _host.assoc_ranksum_host_run.argtypes = [u32, u64, u32, u32, vp, vp, vp, vp, u32, vp, u32, u64, vp, vp, vp, vp, vp, vp]
    return _host


def constant(name: str) -> int:
    """LANES, PERMS_PER_LANE, BLOCK_PERMS, SLICE, GROUP as the kernels have them."""
    return int(getattr(host_lib(), "assoc_ranksum_host_" + name.lower())())


def host_run(planes, offsets, scales, mults, n_samples, case_mask, alternative, edges, permutations, seed):
    """assoc_ranksum_host_run — the primitive's steps on the host: (the five outputs, the four counts)."""
    pl = np.ascontiguousarray(planes, np.uint64).reshape(-1, PLANES)
    off, sc, ml = (np.ascontiguousarray(x, np.uint32) for x in (offsets, scales, mults))
    ed = np.ascontiguousarray(edges, np.uint32)
    F, P, E = len(pl), int(permutations), len(ed)
    alt = ALTERNATIVES.index(alternative) if isinstance(alternative, str) else int(alternative)
    obs, exceed = np.zeros(max(F, 1), np.uint32), np.zeros(max(F, 1), np.uint32)
    labels_, most, tail = np.zeros(max(P, 1), np.uint64), np.zeros(max(P, 1), np.uint32), np.zeros(max(E, 1), np.uint64)
    counts = np.zeros(4, np.uint64)
    rc = host_lib().assoc_ranksum_host_run(int(n_samples), int(case_mask), alt, F, pl.ctypes.data, off.ctypes.data, sc.ctypes.data, ml.ctypes.data,
                                           E, ed.ctypes.data, P, int(seed), obs.ctypes.data, labels_.ctypes.data, most.ctypes.data,
                                           exceed.ctypes.data, tail.ctypes.data, counts.ctypes.data)
    assert rc == 0, rc
    return {"obs_score": obs[:F], "labels": labels_[:P], "perm_max": most[:P], "exceed": exceed[:F], "tail": tail[:E]}, [int(x) for x in counts]


# ---- constructed cases: name -> the contract's arguments (planes, offsets, scales, mults, N, C, alternative, edges, P, seed) ----

def seeded_values(N: int, F: int, seed: int, dense_every=10) -> np.ndarray:
    """F features x N samples of values: most features non-zero in 2 - 4 samples, every dense_every-th in all with ties."""
    rng = np.random.default_rng(seed)
    x = np.zeros((F, N), dtype=np.int64)
    for f in range(F):
        if f % dense_every == 0:
            x[f] = rng.integers(0, max(2, N // 2), size=N)
        else:
            where = rng.choice(N, size=min(N, int(rng.integers(2, 5))), replace=False)
            x[f, where] = rng.integers(1, 4, size=len(where))
    return x


def observed(planes, offsets, scales, N, C_, alt) -> np.ndarray:
    """The observed scores, from the contract itself with no relabeling."""
    return expected_ranksum(planes, offsets, scales, np.ones(len(planes), np.uint32), N, C_, alt, [], 0, 0, clean=True)["obs_score"]


def top_edges(planes, offsets, scales, N, C_, alt, most=MAX_EDGES) -> np.ndarray:
    """The stage's choice: the (up to `most`) largest distinct observed scores, ascending."""
    return np.unique(observed(planes, offsets, scales, N, C_, alt))[-most:].astype(np.uint32)


def case(N, n1, F, P, alt=0, seed=1, value_seed=3, dense_every=10, edges=None, mults=None):
    C_ = au.half_cases(N, n1)
    n1 = bin(C_).count("1")
    x = seeded_values(N, F, value_seed, dense_every)
    planes, off, sc = inputs_of([mid_rank_scores([int(v) for v in row]) for row in x], n1)
    if edges is None:
        edges = top_edges(planes, off, sc, N, C_, alt, 64) if F else np.zeros(0, np.uint32)
    return (planes, off, sc, au.seeded_mults(F, value_seed) if mults is None else mults, N, C_, alt, np.asarray(edges, np.uint32), P, seed)


@functools.lru_cache(maxsize=1)
def constructed() -> dict:
    SLICE, BLOCK_PERMS = constant("slice"), constant("block_perms")
    out = {}
    for N in (2, 3, 31, 32, 33, 63, 64):      # the seam between a word's halves, and a full-width word
        for alt in (0, 1, 2):
            out[f"N{N}_{ALTERNATIVES[alt]}"] = case(N, None, 257, 257, alt, seed=N, dense_every=3 if N < 8 else 10)
    out["N64_one_case"] = case(64, 1, 256, 255, 0, seed=5, dense_every=2)
    out["N64_one_control"] = case(64, 63, 255, 256, 2, seed=6, dense_every=2)
    for F in (0, 1, 255, 256, 257):
        out[f"F{F}"] = case(16, 8, F, 33, F % 3, seed=F)
    for P in (0, 1, 255, 256, 257):
        out[f"P{P}"] = case(16, 8, 40, P, P % 3, seed=P, dense_every=2)
    out["past_a_slice"] = case(20, 9, SLICE + 1, 65, 0, seed=8)
    out["past_a_block_of_relabelings"] = case(20, 9, 65, BLOCK_PERMS + 1, 2, seed=9, dense_every=2)
    out["past_both"] = case(12, 5, SLICE + 1, BLOCK_PERMS + 1, 1, seed=10, dense_every=2)
    out["seed_0"] = case(33, 16, 100, 100, 0, seed=0)
    out["seed_max"] = case(33, 16, 100, 100, 2, seed=(1 << 64) - 1)
    # the kinds of feature, at N = 64: all planes zero; only plane 6; every plane (64 distinct values); one non-zero sample; the
    # case mask's own scores (the cases hold the larger values)
    N, C_ = 64, au.half_cases(64, 32)
    kinds = [[0] * 64, [64 if s % 5 == 0 else 0 for s in range(64)], mid_rank_scores(list(range(64))), mid_rank_scores([0] * 63 + [7]),
             mid_rank_scores([3 if C_ >> s & 1 else 0 for s in range(64)]), mid_rank_scores([s + 100 if C_ >> s & 1 else s for s in range(64)]),
             mid_rank_scores([0, 0] + list(range(1, 63)))]      # (the last: one tie makes the scores above it odd, so every plane is set)
    assert max(kinds[2]) == 126 and planes_of(kinds[1])[:6] == [0] * 6 and all(planes_of(kinds[2])[1:]) and all(planes_of(kinds[6]))
    scores = kinds * 3
    planes, off, sc = inputs_of(scores, 32)
    mults = np.array([1, 2, 0, 4, 5, 6, 7] * 3, dtype=np.uint32)
    for alt in (0, 1, 2):
        out[f"kinds_of_feature_{ALTERNATIVES[alt]}"] = (planes, off, sc, mults, N, C_, alt, top_edges(planes, off, sc, N, C_, alt), 300, 21 + alt)
    # scales of 0 and 2^32 - 1, an offset of 2^32 - 1 (u is clamped at 0 under greater, at 2^20 - 1 under less), multiplicities of
    # 0 and 2^32 - 1 (alone: the sum stays below 2^32)
    planes, off, sc = inputs_of(kinds, 32)
    sc = np.array([0, U32, U32, 0, U32, 1, 77], dtype=np.uint32)
    off2 = off.copy()
    off2[1] = off2[4] = U32
    mults = np.array([0, 0, U32, 0, 0, 0, 0], dtype=np.uint32)
    for alt in (0, 1, 2):
        edges = top_edges(planes, off2, sc, N, C_, alt)
        out[f"extreme_integers_{ALTERNATIVES[alt]}"] = (planes, off2, sc, mults, N, C_, alt, edges, 257, 31)
    # three equal features whose multiplicities sum to 2^32 - 1 at P = 257 with edges = [0]: one cell holds every pair, past 2^32
    planes, off, sc = inputs_of([kinds[5], kinds[1], kinds[5], kinds[5]], 32)
    mults = np.array([1 << 31, 0, (1 << 31) - 2, 1], dtype=np.uint32)
    out["three_equal_sum_to_2_32_less_1"] = (planes, off, sc, mults, N, C_, 0, np.zeros(1, np.uint32), 257, 41)
    # E of 0, 1 and 1024, and edges all above every score
    base = case(24, 11, 300, 300, 2, seed=51, dense_every=2)
    top = int(observed(*base[:3], 24, base[5], 2).max())
    out["E0"] = base[:7] + (np.zeros(0, np.uint32),) + base[8:]
    out["E1"] = base[:7] + (np.array([top // 3], np.uint32),) + base[8:]
    out["E1024"] = base[:7] + ((np.arange(1024, dtype=np.uint32) * np.uint32(max(1, top // 600)) + np.uint32(1)),) + base[8:]
    out["edges_above_every_score"] = base[:7] + (np.array([U32 - 2, U32 - 1, U32], np.uint32),) + base[8:]
    # contention: every feature the case mask's own scores, every block raises the same perm_max and adds to one tail cell
    planes, off, sc = inputs_of([kinds[4]] * (2 * SLICE + 3), 32)
    out["every_feature_the_same"] = (planes, off, sc, np.full(2 * SLICE + 3, 3, np.uint32), N, C_, 2, np.array([0, 5], np.uint32), BLOCK_PERMS + 7, 14)
    base = case(16, 8, 300, 300, 0, seed=15)
    out["all_multiplicities_0"] = base[:3] + (np.zeros(300, np.uint32),) + base[4:]
    return out


def constructed_names() -> list:
    return list(constructed())


def premise(name: str, args, want):
    """What a constructed case is for, checked on the contract's own result."""
    planes, off, sc, mults, N, C_, alt, edges, P, seed = args
    if name == "three_equal_sum_to_2_32_less_1":
        assert int(mults.astype(np.uint64).sum()) == U32 and int(want["tail"][0]) == U32 * P > 1 << 32
    if name.startswith("extreme_integers"):
        assert int(want["tail"].sum(dtype=object)) >= 1 << 32 and int(want["obs_score"][0]) == int(want["obs_score"][3]) == 0      # scale 0
    if name == "extreme_integers_less":
        assert int(want["obs_score"][1]) == (((1 << SHIFT) - 1) * U32) >> SHIFT      # u clamped at the top, the largest score there is
    if name == "extreme_integers_greater":
        assert int(want["obs_score"][1]) == 0      # u clamped at 0
    if name == "all_multiplicities_0":
        assert not want["perm_max"].any() and not want["tail"].any() and want["exceed"].any()      # exceed counts every feature
    if name == "E0":
        assert len(want["tail"]) == 0
    if name == "E1024":
        assert len(want["tail"]) == 1024 and np.count_nonzero(want["tail"]) > 100
    if name == "edges_above_every_score":
        assert not want["tail"].any() and want["perm_max"].any()
    if name == "every_feature_the_same":
        assert (want["labels"] == np.uint64(C_)).sum() >= 0 and len(set(want["exceed"].tolist())) == 1
    if name.startswith("N") or name.startswith("kinds"):
        assert want["exceed"].any() and want["perm_max"].any()


# ---- the stage's files, from their definitions ----

def six_e(x) -> str:
    return "." if x is None else format(float(x), ".6e")


def stage_files(identity, rows, x_rows, N, case_mask, alternative: str, P: int, result, depths=None):
    """(associate.tsv, associate_null.tsv) as bytes from per-feature identity cells (bytes), the features' values over the used
    samples (already cut at --min-count) and the null's result on ONE ROW PER FEATURE with multiplicity 1 (None: no
    permutations) — every column from its definition, feature by feature."""
    alt = ALTERNATIVES.index(alternative)
    n1 = bin(case_mask).count("1")
    n0 = N - n1
    feats = []
    for f, x in enumerate(x_rows):
        a = mid_rank_scores(x, depths)
        A, B, Q, offset, scale = sums(a, n1)
        D = N * sum(v for s, v in enumerate(a) if case_mask >> s & 1) - offset
        feats.append({"f": f, "x": x, "a": a, "D": D, "Q": Q, "t": score(D, scale, alt)})
    edges = sorted({ft["t"] for ft in feats})[-MAX_EDGES:]

    def O(e):
        return sum(1 for ft in feats if ft["t"] >= e)

    def V(e):
        return sum(int(result["tail"][j]) for j, other in enumerate(edges) if other >= e)

    def fdr(e):
        return min(Fraction(1), Fraction(V(e), P * O(e))) if O(e) else None
    head = ["nonzero", "nonzero_cases", "nonzero_controls", "cases", "controls", "mean_rank_cases", "mean_rank_controls", "z", "score", "p_value",
            "p_adjusted", "q_value"]
    lines = ["\t".join(identity + head).encode()]
    for ft in sorted(feats, key=lambda ft: (-ft["t"], ft["f"])):
        x, t = ft["x"], ft["t"]
        if depths is None:
            mid = [(2 * sum(v < w for v in x) + sum(v == w for v in x) + 1) / 2 for w in x]      # the mid-ranks themselves
        else:
            key = [Fraction(v, d) if v else Fraction(0) for v, d in zip(x, depths)]
            mid = [(2 * sum(v < w for v in key) + sum(v == w for v in key) + 1) / 2 for w in key]
        in_cases = [bool(case_mask >> s & 1) for s in range(N)]
        cells = [str(sum(v > 0 for v in x)), str(sum(v > 0 and c for v, c in zip(x, in_cases))), str(sum(v > 0 and not c for v, c in zip(x, in_cases))),
                 str(n1), str(n0), format(sum(m for m, c in zip(mid, in_cases) if c) / n1, ".6g"),
                 format(sum(m for m, c in zip(mid, in_cases) if not c) / n0, ".6g"),
                 "nan" if ft["Q"] == 0 else format(z_of(ft["D"], ft["Q"], N, n1), ".6g"), str(t)]
        if result is not None:
            p = Fraction(1 + int(result["exceed"][ft["f"]]), P + 1)
            adj = Fraction(1 + sum(1 for v in result["perm_max"] if int(v) >= t), P + 1)
            below = [x_ for x_ in (fdr(e) for e in edges if e <= t) if x_ is not None]
            cells += [six_e(p), six_e(adj), six_e(min(below) if below else None)]
        else:
            cells += ["."] * 3
        lines.append(rows[ft["f"]] + b"\t" + "\t".join(cells).encode())
    null = ["\t".join(["score", "z", "features", "features_cumulative", "null_pairs", "null_cumulative", "expected_false", "fdr"]).encode()]
    for j in range(len(edges) - 1, -1, -1):
        e = edges[j]
        cells = [str(e), format(e / float(1 << (32 - SHIFT)) * sqrt((N - 1) / (n1 * n0)), ".6g"), str(sum(1 for ft in feats if ft["t"] == e)), str(O(e))]
        if result is not None:
            cells += [str(int(result["tail"][j])), str(V(e)), format(float(Fraction(V(e), P)), ".6g"), six_e(fdr(e))]
        else:
            cells += ["."] * 4
        null.append("\t".join(cells).encode())
    return b"\n".join(lines) + b"\n", b"\n".join(null) + b"\n", feats, edges


# ---- the hand-written cohort of the stage tests: assoc_util's 18 samples (16 used, 8 cases) with features for an abundance test ----

SAMPLES, USED, CASES, UNKNOWN, NOT_IN_PH = au.SAMPLES, au.USED, au.CASES, au.UNKNOWN, au.NOT_IN_PH
CONTROLS = [s for s in USED if s not in CASES]
# name -> the samples it occurs in with (clonotypes, reads); everyone else has (0, 0)
FEATURES = [
    ("separates_completely", {**{s: (5 + i, 50 + i) for i, s in enumerate(CASES)}, **{s: (1, 2 + i) for i, s in enumerate(CONTROLS)}}),
    ("constant", {s: (2, 6) for s in SAMPLES}),
    ("all_zero", {}),
    ("same_scores_a", {CASES[0]: (1, 2), CASES[1]: (3, 4), CONTROLS[0]: (2, 3)}),
    ("same_scores_b", {CASES[0]: (10, 20), CASES[1]: (30, 40), CONTROLS[0]: (20, 30)}),
    ("deeper_in_controls", {**{s: (4, 9) for s in CONTROLS[:6]}, CASES[2]: (1, 1), CASES[5]: (1, 12)}),
    ("present_everywhere_expanded_in_cases", {**{s: (3, 30) for s in CASES[:6]}, **{s: (1, 1) for s in USED if s not in CASES[:6]}, UNKNOWN: (9, 9), NOT_IN_PH: (7, 7)}),
    ("one_sample", {CASES[7]: (2, 1)}),
]
# depths that reverse the raw order of the constant feature's neighbours: the cases are sequenced ten times as deep
DEPTHS = {s: ((1000, 10000) if s in CASES else (100, 1000)) for s in SAMPLES}


def tabulate_text() -> bytes:
    head = ["metaclonotype", "v_call", "j_call", "junction_aa", "radius", "samples"] + [f"{s}_{w}" for s in SAMPLES for w in ("clonotypes", "reads")]
    lines = ["\t".join(head)]
    for n, (name, where) in enumerate(FEATURES):
        cells = [str(n * 3), f"TRBV{n + 2}*01", "TRBJ2-1*01", "CASS" + name.upper().replace("_", "") + "F", str(12 + 2 * n), str(len(where))]
        for s in SAMPLES:
            cells += [str(where.get(s, (0, 0))[0]), str(where.get(s, (0, 0))[1])]
        lines.append("\t".join(cells))
    return ("\n".join(lines) + "\n").encode()


def public_text() -> bytes:
    head = ["v_call", "j_call", "junction_aa", "n_samples", "duplicate_count"] + SAMPLES
    lines = ["\t".join(head)]
    for n, (name, where) in enumerate(FEATURES):
        cells = [f"TRBV{n + 2}*01", "TRBJ2-1*01", "CASS" + name.upper().replace("_", "") + "F", str(len(where)), str(sum(v[1] for v in where.values()))]
        cells += [str(where.get(s, (0, 0))[1]) for s in SAMPLES]
        lines.append("\t".join(cells))
    return ("\n".join(lines) + "\n").encode()


def samples_text() -> bytes:
    """A tabulate_samples.tsv as `tabulate` writes it, holding DEPTHS."""
    lines = ["sample\tclonotypes\treads\ttake_part\tclonotypes_inside\treads_inside\tmetaclonotypes_found"]
    lines += [f"{s}\t{DEPTHS[s][0]}\t{DEPTHS[s][1]}\t1\t0\t0\t0" for s in SAMPLES]
    return ("\n".join(lines) + "\n").encode()


def identity_rows(kind: str):
    text = tabulate_text() if kind == "tabulate" else public_text()
    width = 5 if kind == "tabulate" else 3
    lines = text.split(b"\n")[:-1]
    return [h.decode() for h in lines[0].split(b"\t")[:width]], [b"\t".join(x.split(b"\t")[:width]) for x in lines[1:]]


def hand_values(value: str, min_count: int) -> list:
    """The features' values over USED, cut at min_count — from FEATURES, not from the files."""
    at = 0 if value == "clonotypes" else 1
    return [[(where.get(s, (0, 0))[at] if where.get(s, (0, 0))[at] >= min_count else 0) for s in USED] for _, where in FEATURES]


def hand_depths(value: str) -> list:
    return [DEPTHS[s][0 if value == "clonotypes" else 1] for s in USED]


def hand_null(x_rows, alternative: str, P: int, seed: int, depths=None) -> dict:
    """The contract on one row per feature, multiplicity 1, with the edges the stage picks."""
    scores = [mid_rank_scores(x, depths) for x in x_rows]
    planes, off, sc = inputs_of(scores, 8)
    alt = ALTERNATIVES.index(alternative)
    edges = top_edges(planes, off, sc, 16, au.HAND_CASE_MASK, alt)
    return expected_ranksum(planes, off, sc, np.ones(len(scores), np.uint32), 16, au.HAND_CASE_MASK, alt, edges, P, seed)
