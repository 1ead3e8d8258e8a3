"""What the association tests share (`associate`; include/dcrx.h "association"): the contract as Python that shares no method with
the kernels — the exact test from the hypergeometric point probabilities in Fractions, dense ranks, a relabeling as the n1
smallest of N sorted keys (tests/rarefy_util.key), the null as numpy popcounts over whole arrays —, the stage's derived columns
from their definitions, the constructed cases, the stand-in for the native call, the hand-written tables of the stage tests and
the host build of the shared code and of the primitive's steps (tests/host_assoc)."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction
from math import comb

import numpy as np

from tests import rarefy_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_assoc")
HOST_LIB = os.path.join(HOST_DIR, "build", "libassoc_host.so")
OUTPUTS = ("obs_rank", "labels", "perm_min", "tail")
STATS = ("features", "features_weighted", "weight", "permutations", "tail_total", "min_perm_rank")
ALTERNATIVES = ("greater", "less", "two-sided")
MAX_SAMPLES, MAX_PERMUTATIONS, MAX_FEATURES, MAX_WEIGHT = 64, 1 << 20, 1 << 30, 1 << 32
NO_RANK = 0xFFFF


class Invalid(Exception):
    """What the contract answers with DCRX_E_INVALID."""


class Unsupported(Exception):
    """What the contract answers with DCRX_E_UNSUPPORTED."""


# ---- the test ----

def feasible(N: int, n1: int, m: int) -> range:
    return range(max(0, m - (N - n1)), min(m, n1) + 1)


def fisher_table(N: int, n1: int, alternative: str) -> dict:
    """{(m, k): p} over the feasible cells, p the exact Fraction: the point probabilities of the hypergeometric distribution,
    each a Fraction of its own, summed over the alternative's side."""
    out = {}
    for m in range(N + 1):
        pmf = {x: Fraction(comb(n1, x) * comb(N - n1, m - x), comb(N, m)) for x in feasible(N, n1, m)}
        for k in pmf:
            if alternative == "greater":
                out[(m, k)] = sum((q for x, q in pmf.items() if x >= k), Fraction(0))
            elif alternative == "less":
                out[(m, k)] = sum((q for x, q in pmf.items() if x <= k), Fraction(0))
            elif alternative == "two-sided":
                out[(m, k)] = sum((q for q in pmf.values() if q <= pmf[k]), Fraction(0))
            else:
                raise ValueError(alternative)
    return out


@functools.lru_cache(maxsize=32)
def rank_table(N: int, n1: int, alternative: str):
    """(table, p_of_rank): (N + 1)^2 uint16, m-major, dense ranks of the p-values (NO_RANK where no cohort gets), read only."""
    cells = fisher_table(N, n1, alternative)
    p_of_rank = sorted(set(cells.values()))
    table = np.full((N + 1) * (N + 1), NO_RANK, dtype=np.uint16)
    for (m, k), p in cells.items():
        table[m * (N + 1) + k] = p_of_rank.index(p)
    table.setflags(write=False)
    return table, tuple(p_of_rank)


@functools.lru_cache(maxsize=32)
def census_table(N: int, n1: int):
    """A table in which every feasible cell has a rank of its own (numbered m ascending, k DEScending: not monotone the way a
    one-sided test is): with tail_ranks = n_ranks the tail is the (m, k) census.  (table, n_ranks), read only."""
    table = np.full((N + 1) * (N + 1), NO_RANK, dtype=np.uint16)
    n = 0
    for m in range(N + 1):
        for k in reversed(feasible(N, n1, m)):
            table[m * (N + 1) + k] = n
            n += 1
    table.setflags(write=False)
    return table, n


# ---- the contract ----

def popcount(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.int64)
    return np.unpackbits(x.reshape(-1, 1).view(np.uint8), axis=1).sum(axis=1).reshape(x.shape).astype(np.int64)


def labels(seed: int, p: int, N: int, n1: int) -> int:
    """L_p: the n1 samples with the smallest key(seed, p, s)."""
    order = sorted(range(N), key=lambda s: ru.key(seed, p, s))
    return sum(1 << s for s in order[:n1])


def labels_numpy(seed: int, P: int, N: int, n1: int) -> np.ndarray:
    """labels() for p = 0 .. P - 1 at once: the keys in numpy uint64 arithmetic, an argsort per relabeling."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.arange(1, P + 1, dtype=np.uint64) * u(ru.SAMPLE_STEP) + u(seed)
        for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
            z ^= z >> u(shift); z *= u(mul)
        z ^= z >> u(31)
        z = z[:, None] + np.arange(1, N + 1, dtype=np.uint64)[None, :] * u(ru.READ_STEP)
        for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
            z ^= z >> u(shift); z *= u(mul)
        z ^= z >> u(31)
    first = np.argsort(z, axis=1, kind="stable")[:, :n1].astype(np.uint64)
    return np.bitwise_or.reduce(u(1) << first, axis=1) if P else np.zeros(0, np.uint64)


def refuse(N, C, F, n_ranks, tail_ranks, P):
    """The scalars, in the header's order."""
    if not 2 <= N <= MAX_SAMPLES:
        raise Invalid("samples")
    if C >> N or C == 0 or C == (1 << N) - 1:
        raise Invalid("case mask")
    if n_ranks == 0 or n_ranks > (N + 1) ** 2 or tail_ranks > n_ranks:
        raise Invalid("ranks")
    if F >= MAX_FEATURES or P > MAX_PERMUTATIONS:
        raise Unsupported("size")


def expected_permute(masks, mults, n_samples, case_mask, table, n_ranks, tail_ranks, permutations, seed, clean=False) -> dict:
    """The contract of dcrx_assoc_permute (clean: the device entry's — masks are cut to N bits and nothing of the arrays is
    refused)."""
    N, C_, P, T = int(n_samples), int(case_mask), int(permutations), int(tail_ranks)
    masks, mults = np.asarray(masks, dtype=np.uint64), np.asarray(mults, dtype=np.uint64)
    table = np.asarray(table, dtype=np.uint16).reshape(-1)
    F = len(masks)
    refuse(N, C_, F, n_ranks, T, P)
    n1 = bin(C_).count("1")
    bits = np.uint64((1 << N) - 1)
    if clean:
        masks = masks & bits
    else:
        if F and int((masks & ~bits).max()):
            raise Invalid("a mask with a bit at or above N")
        for m in range(N + 1):
            if any(int(table[m * (N + 1) + k]) >= n_ranks for k in feasible(N, n1, m)):
                raise Invalid("a feasible cell at or above n_ranks")
        if int(mults.sum(dtype=object) if F else 0) >= MAX_WEIGHT:
            raise Unsupported("multiplicity sum")
    m = popcount(masks)
    obs = table[m * (N + 1) + popcount(masks & np.uint64(C_))].astype(np.uint32)
    L = labels_numpy(seed, P, N, n1)
    least = np.full(P, n_ranks, dtype=np.uint32)
    tail = np.zeros(T, dtype=np.uint64)
    part = mults > 0
    if part.any() and P:
        mk, w, row = masks[part], mults[part], m[part] * (N + 1)
        lo, hi = (w & np.uint64(0xFFFF)).astype(np.float64), (w >> np.uint64(16)).astype(np.float64)      # exact in float64 sums
        for a in range(0, P, 256):
            r = table[row[None, :] + popcount(mk[None, :] & L[a:a + 256, None])].astype(np.int64)
            least[a:a + 256] = r.min(axis=1)
            inside = r < T
            if T and inside.any():
                rr = r[inside]
                ww = np.broadcast_to(lo, r.shape)[inside], np.broadcast_to(hi, r.shape)[inside]
                tail += np.bincount(rr, ww[0], T).astype(np.uint64) + (np.bincount(rr, ww[1], T).astype(np.uint64) << np.uint64(16))
    stats = {"features": F, "features_weighted": int(part.sum()), "weight": int(mults.sum(dtype=object)) if F else 0, "permutations": P,
             "tail_total": int(tail.sum(dtype=object)) if T else 0, "min_perm_rank": int(least.min()) if P else n_ranks}
    return {"obs_rank": obs, "labels": L, "perm_min": least, "tail": tail, "stats": stats}


def assert_same(got: dict, want: dict, what=""):
    for key in OUTPUTS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        assert np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, key, np.flatnonzero(g.astype(np.uint64) != w.astype(np.uint64))[:8])


def python_permute(calls=None):
    """The stand-in for nat.assoc_permute: the contract, with a record of the calls."""
    def run(*args):
        if calls is not None:
            calls.append(args)
        return expected_permute(*args)
    return run


# ---- the host build (tests/host_assoc) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", HOST_DIR])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        for name in ("lanes", "perms_per_lane", "block_perms", "slice", "max_samples", "max_permutations"):
            getattr(_host, "assoc_host_" + name).restype = u32
        _host.assoc_host_select_labels.restype, _host.assoc_host_select_labels.argtypes = u64, [u64, u32, u32, u32]
        _host.assoc_host_score.restype, _host.assoc_host_score.argtypes = u32, [vp, u32, u64, u64]
        _host.assoc_host_feasible.restype, _host.assoc_host_feasible.argtypes = C.c_int, [u32, u32, u32, u32]
        _host.assoc_host_refuse.restype, _host.assoc_host_refuse.argtypes = C.c_int, [u32, u64, u64, u32, u32, u32]
        _host.assoc_host_permute.restype = C.c_int
        _host.assoc_host_permute.argtypes = [u32, u64, u32, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, vp]
    return _host


def constant(name: str) -> int:
    """LANES, PERMS_PER_LANE, BLOCK_PERMS, SLICE as the kernels have them."""
    return int(getattr(host_lib(), "assoc_host_" + name.lower())())


def host_permute(masks, mults, n_samples, case_mask, table, n_ranks, tail_ranks, permutations, seed):
    """assoc_host_permute — the primitive's steps on the host: (the four outputs, the blocks' flushes)."""
    mk, ml = np.ascontiguousarray(masks, np.uint64), np.ascontiguousarray(mults, np.uint32)
    tb = np.ascontiguousarray(table, np.uint16)
    F, P, T = len(mk), int(permutations), int(tail_ranks)
    obs, labels_, least = np.zeros(max(F, 1), np.uint32), np.zeros(max(P, 1), np.uint64), np.zeros(max(P, 1), np.uint32)
    tail, flushes = np.zeros(max(T, 1), np.uint64), C.c_uint64(0)
    rc = host_lib().assoc_host_permute(int(n_samples), int(case_mask), F, mk.ctypes.data, ml.ctypes.data, tb.ctypes.data, int(n_ranks), T, P,
                                       int(seed), obs.ctypes.data, labels_.ctypes.data, least.ctypes.data, tail.ctypes.data, C.byref(flushes))
    assert rc == 0, rc
    return {"obs_rank": obs[:F], "labels": labels_[:P], "perm_min": least[:P], "tail": tail[:T]}, int(flushes.value)


# ---- constructed cases: name -> the arguments of the contract (masks, mults, N, C, table, n_ranks, tail_ranks, P, seed) ----

def seeded_masks(N: int, F: int, seed: int, sparse=True) -> np.ndarray:
    """F presence patterns of N samples: most features in a few samples (the AND of three draws), every tenth dense."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(3, F), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(3, F), dtype=np.uint64)
    out = a[0] & a[1] & a[2] if sparse else a[0].copy()
    out[::10] = a[0][::10]
    return out & np.uint64((1 << N) - 1)


def seeded_mults(F: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed + 1)
    w = rng.integers(1, 1000, size=F, dtype=np.uint64).astype(np.uint32)
    w[::7] = 0
    return w


def half_cases(N: int, n1=None) -> int:
    """A case mask of n1 (default N // 2) cases spread over the samples: every other sample first, then from the top."""
    n1 = N // 2 if n1 is None else n1
    picked = []
    for s in list(range(0, N, 2)) + list(range(N - 1, -1, -1)):
        if s not in picked:
            picked.append(s)
    return sum(1 << s for s in picked[:n1])


def table_for(kind: str, N: int, n1: int):
    """(table, n_ranks, tail_ranks) of the three kinds of table: greater and two-sided with the ranks at or below 1/20 as the
    tail, census with every rank in the tail."""
    if kind == "census":
        table, n = census_table(N, n1)
        return table, n, n
    table, p_of_rank = rank_table(N, n1, kind)
    return table, len(p_of_rank), sum(p <= Fraction(1, 20) for p in p_of_rank)


def case(N, n1, F, P, kind="census", seed=1, mask_seed=3, sparse=True, tail_ranks=None):
    C_ = half_cases(N, n1)
    table, n_ranks, tail = table_for(kind, N, bin(C_).count("1"))
    return (seeded_masks(N, F, mask_seed, sparse), seeded_mults(F, mask_seed), N, C_, table, n_ranks, tail if tail_ranks is None else tail_ranks, P, seed)


@functools.lru_cache(maxsize=1)
def constructed() -> dict:
    SLICE, BLOCK_PERMS = constant("slice"), constant("block_perms")
    out = {}
    for N in (2, 3, 31, 32, 33, 63, 64):      # the seam between a mask's halves, and a full-width mask
        for kind in ("greater", "two-sided", "census"):
            out[f"N{N}_{kind}"] = case(N, None, 257, 257, kind, seed=N, sparse=N > 8)
    for N in (2, 33, 64):
        out[f"N{N}_one_case"] = case(N, 1, 256, 255, "census", seed=5, sparse=False)
        out[f"N{N}_one_control"] = case(N, N - 1, 255, 256, "census", seed=6, sparse=False)
    for F in (0, 1, 255, 256, 257):
        out[f"F{F}"] = case(16, 8, F, 33, "census", seed=F)
    for P in (0, 1, 255, 256, 257):
        out[f"P{P}"] = case(16, 8, 40, P, "two-sided", seed=P, sparse=False)
    out["past_a_slice"] = case(20, 9, SLICE + 1, 65, "census", seed=8)
    out["past_a_block_of_relabelings"] = case(20, 9, 65, BLOCK_PERMS + 1, "census", seed=9, sparse=False)
    out["past_both"] = case(12, 5, SLICE + 1, BLOCK_PERMS + 1, "greater", seed=10, sparse=False)
    out["tail_0"] = case(16, 8, 100, 100, "greater", seed=11, sparse=False, tail_ranks=0)
    out["tail_1"] = case(16, 8, 100, 100, "greater", seed=12, sparse=False, tail_ranks=1)
    out["seed_0"] = case(33, 16, 100, 100, "census", seed=0)
    out["seed_max"] = case(33, 16, 100, 100, "census", seed=(1 << 64) - 1)
    # multiplicities: 0 and 2^32 - 1, and three features of one mask that sum to 2^32 - 1 at P = 257: a tail cell passes 2^32
    masks, mults, N, C_, table, n_ranks, tail, P, seed = case(16, 8, 8, 257, "census", seed=13, sparse=False)
    mults = np.array([0, (1 << 32) - 1, 0, 0, 0, 0, 0, 0], dtype=np.uint32)
    out["one_full_multiplicity"] = (masks, mults, N, C_, table, n_ranks, tail, P, seed)
    masks = masks.copy()
    masks[2] = masks[5] = masks[7] = np.uint64(0x0F0F)
    mults = np.array([0, 0, 1 << 31, 0, 0, (1 << 31) - 2, 0, 1], dtype=np.uint32)
    out["three_of_one_mask_sum_to_2_32_less_1"] = (masks, mults, N, C_, table, n_ranks, tail, P, seed)
    # contention: every feature is the case mask itself and (n1, n1) is in the tail — every lane of every wave adds to one cell
    # where L_p = C, and every block lowers the same perm_min
    N, C_ = 6, 0b000111
    table, n_ranks, tail = table_for("greater", N, 3)
    out["every_feature_is_the_case_mask"] = (np.full(2 * SLICE + 3, C_, dtype=np.uint64), np.full(2 * SLICE + 3, 3, dtype=np.uint32), N, C_,
                                             table, n_ranks, max(tail, 1), BLOCK_PERMS + 7, 14)
    masks, mults, N, C_, table, n_ranks, tail, P, seed = case(16, 8, 300, 300, "census", seed=15)
    out["all_multiplicities_0"] = (masks, np.zeros(300, np.uint32), N, C_, table, n_ranks, tail, P, seed)
    return out


def constructed_names() -> list:
    return list(constructed())


def premise(name: str, args, want):
    """What a constructed case is for, checked on the contract's own result."""
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = args
    if name == "three_of_one_mask_sum_to_2_32_less_1":
        assert int(mults.astype(np.uint64).sum()) == (1 << 32) - 1 and int(want["tail"].max()) >= 1 << 32
    if name == "one_full_multiplicity":
        assert int(want["tail"].max()) >= 1 << 32
    if name == "every_feature_is_the_case_mask":
        assert int(table[3 * (N + 1) + 3]) < tail_ranks and (want["labels"] == np.uint64(C_)).sum() > 1 and want["perm_min"].min() == 0
    if name == "all_multiplicities_0":
        assert (want["perm_min"] == n_ranks).all() and not want["tail"].any()
    if name.endswith("_census") or name.startswith(("F", "past_a")):
        assert tail_ranks == n_ranks and int(want["tail"].sum()) == int(mults.astype(np.uint64).sum()) * P      # every pair is in the census
    if name == "tail_0":
        assert len(want["tail"]) == 0
    if name in ("N32_two-sided", "N64_two-sided"):
        n1 = bin(C_).count("1")
        row = [int(table[10 * (N + 1) + k]) for k in feasible(N, n1, 10)]
        assert row != sorted(row) and row != sorted(row, reverse=True)      # not monotone in k


# ---- the stage's derived columns, from their definitions ----

def six_e(x) -> str:
    return "." if x is None else format(float(x), ".6e")


def stage_files(identity, rows, masks, N, case_mask, alternative, max_p: Fraction, P: int, result):
    """(associate.tsv, associate_null.tsv) as bytes from per-feature identity cells (bytes), the features' masks over the used
    samples and the null's result (None: no permutations) — every column from its definition, feature by feature."""
    n1 = bin(case_mask).count("1")
    n0 = N - n1
    p_of = fisher_table(N, n1, alternative)
    p_of_rank = sorted(set(p_of.values()))
    feats = []
    for f, M in enumerate(int(x) for x in masks):
        m, k = bin(M).count("1"), bin(M & case_mask).count("1")
        feats.append((p_of_rank.index(p_of[(m, k)]), f, m, k))
    tail_ranks = sum(p <= max_p for p in p_of_rank)

    def O(r):
        return sum(1 for rank, *_ in feats if rank <= r)

    def V(r):
        return sum(int(x) for x in result["tail"][:r + 1])

    def fdr(r):
        return min(Fraction(1), Fraction(V(r), P * O(r))) if O(r) else None
    lines = ["\t".join(identity + ["present", "present_cases", "present_controls", "cases", "controls", "odds_ratio", "p_value",
                                   "p_adjusted", "q_value"]).encode()]
    for rank, f, m, k in sorted(feats):
        num, den = k * (n0 - m + k), (m - k) * (n1 - k)
        ratio = ("inf" if num else "nan") if den == 0 else format(float(Fraction(num, den)), ".6g")
        adj = q = None
        if result is not None:
            adj = Fraction(1 + sum(1 for x in result["perm_min"] if int(x) <= rank), P + 1)
            if rank < tail_ranks:
                q = min(x for x in (fdr(r) for r in range(rank, tail_ranks)) if x is not None)
        cells = [str(m), str(k), str(m - k), str(n1), str(n0), ratio, six_e(p_of_rank[rank]), six_e(adj), six_e(q)]
        lines.append(rows[f] + b"\t" + "\t".join(cells).encode())
    null = ["\t".join(["rank", "p_value", "features", "features_cumulative", "null_pairs", "null_cumulative", "expected_false", "fdr"]).encode()]
    for r in range(tail_ranks):
        cells = [str(r), six_e(p_of_rank[r]), str(sum(1 for rank, *_ in feats if rank == r)), str(O(r))]
        if result is not None:
            cells += [str(int(result["tail"][r])), str(V(r)), format(float(Fraction(V(r), P)), ".6g"), six_e(fdr(r))]
        else:
            cells += ["."] * 4
        null.append("\t".join(cells).encode())
    return b"\n".join(lines) + b"\n", b"\n".join(null) + b"\n"


# ---- the hand-written cohort of the stage tests: 16 samples used (8 cases), one with group `.`, one missing from -ph ----

SAMPLES = [f"S{i:02d}" for i in range(18)]
UNKNOWN, NOT_IN_PH = "S05", "S11"
USED = [s for s in SAMPLES if s not in (UNKNOWN, NOT_IN_PH)]
CASES = USED[:3] + USED[8:13]      # 8 of the 16: not a prefix of the columns
# name -> (the samples it is present in with (clonotypes, reads); everyone else has (0, 0))
FEATURES = [
    ("exactly_the_cases", {s: (2, 9) for s in CASES}),
    ("everywhere", {s: (1, 3) for s in SAMPLES}),
    ("nowhere", {}),
    ("one_mask_a", {CASES[0]: (1, 2), CASES[1]: (3, 4), USED[4]: (1, 1)}),
    ("one_mask_b", {CASES[0]: (5, 5), CASES[1]: (1, 7), USED[4]: (2, 2)}),
    ("mostly_controls", {s: (1, 2) for s in USED if s not in CASES} | {CASES[2]: (1, 1)}),
    ("one_read_somewhere", {CASES[3]: (1, 1), CASES[4]: (1, 2), USED[5]: (1, 1), UNKNOWN: (4, 4), NOT_IN_PH: (2, 6)}),
]


def phenotype_text(extra_columns=True) -> bytes:
    lines = ["donor\tsample\tage\tgroup" if extra_columns else "sample\tgroup"]
    for i, s in enumerate(SAMPLES):
        if s == NOT_IN_PH:
            continue
        group = "." if s == UNKNOWN else ("CMV+" if s in CASES else "CMV-")
        lines.append(f"d{i}\t{s}\t{30 + i}\t{group}" if extra_columns else f"{s}\t{group}")
    return ("\n".join(lines) + "\n").encode()


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


def identity_rows(kind: str):
    """(identity column names, per feature the identity cells joined by tabs) of the two hand-written tables."""
    text = tabulate_text() if kind == "tabulate" else public_text()
    width = 5 if kind == "tabulate" else 3
    lines = text.split(b"\n")[:-1]
    return [h.decode() for h in lines[0].split(b"\t")[:width]], [b"\t".join(x.split(b"\t")[:width]) for x in lines[1:]]


def hand_masks(value: str, min_count: int) -> np.ndarray:
    """The features' presence over USED (bit i: USED[i]) — from FEATURES, not from the files."""
    at = 0 if value == "clonotypes" else 1
    return np.array([sum(1 << i for i, s in enumerate(USED) if where.get(s, (0, 0))[at] >= min_count) for _, where in FEATURES], dtype=np.uint64)


HAND_CASE_MASK = sum(1 << i for i, s in enumerate(USED) if s in CASES)
