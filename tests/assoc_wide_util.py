"""What the wide association tests share (`associate` on 65 to 1024 samples; include/dcrx.h "association, wide"): the contract as
plain Python over big integers — a presence pattern and a relabeling are ONE Python integer of N bits each, a relabeling the n1
smallest of N sorted keys (tests/rarefy_util.key), the null a double loop over relabelings and features —, the constructed cases,
the stand-in for the native call, the hand-written 70-sample cohort in two tabulate.tsv files and the host build of the shared
code and of the primitive's steps (tests/host_assoc_wide).  tests/assoc_util.py holds the narrow layer's and is imported as it is."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from tests import assoc_util as au
from tests import rarefy_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_DIR = os.path.join(HERE, "host_assoc_wide")
HOST_LIB = os.path.join(HOST_DIR, "build", "libassoc_wide_host.so")
HOST_MAIN = os.path.join(HOST_DIR, "build", "assoc_wide_main")
OUTPUTS = au.OUTPUTS
MAX_SAMPLES, MAX_PERMUTATIONS, MAX_FEATURES, MAX_WEIGHT = 1024, 1 << 20, 1 << 30, 1 << 32
NO_RANK = 0xFFFFFFFF
WORD = (1 << 64) - 1
Invalid, Unsupported = au.Invalid, au.Unsupported


# ---- words and integers ----

def words_for(N: int) -> int:
    return (N + 63) // 64


def to_int(words) -> int:
    """W words (sample s: bit s & 63 of word s >> 6) as one integer (sample s: bit s)."""
    return sum(int(x) << (64 * w) for w, x in enumerate(np.asarray(words, dtype=np.uint64).reshape(-1)))


def to_words(x: int, W: int) -> np.ndarray:
    return np.array([(x >> (64 * w)) & WORD for w in range(W)], dtype=np.uint64)


def rows_of(ints, W: int) -> np.ndarray:
    """Integers of up to 64 W bits as an F x W array of words."""
    return np.array([[(x >> (64 * w)) & WORD for w in range(W)] for x in ints], dtype=np.uint64).reshape(len(ints), W)


# ---- the contract ----

def label(seed: int, p: int, N: int, n1: int) -> int:
    """L_p as one integer: the n1 samples with the smallest key(seed, p, s)."""
    order = sorted(range(N), key=lambda s: ru.key(seed, p, s))
    return sum(1 << s for s in order[:n1])


@functools.lru_cache(maxsize=64)
def labels(seed: int, P: int, N: int, n1: int) -> tuple:
    """L_p for p = 0 .. P - 1."""
    return tuple(label(seed, p, N, n1) for p in range(P))


def refuse(N, F, n_ranks, tail_ranks, P):
    """The scalars, in the header's order."""
    if not 2 <= N <= MAX_SAMPLES:
        raise Invalid("samples")
    if n_ranks == 0 or n_ranks > (N + 1) ** 2 or tail_ranks > n_ranks:
        raise Invalid("ranks")
    if F >= MAX_FEATURES or P > MAX_PERMUTATIONS:
        raise Unsupported("size")


def expected_permute_wide(masks, mults, n_samples, case_words, table, n_ranks, tail_ranks, permutations, seed, clean=False) -> dict:
    """The contract of dcrx_assoc_permute_wide (clean: the device entry's — the case mask and the masks are cut to N bits and
    nothing of the arrays is refused).  masks: F x W words (or F words where W is 1); case_words: W words or one integer."""
    N, P, T = int(n_samples), int(permutations), int(tail_ranks)
    masks = np.asarray(masks, dtype=np.uint64)
    F = len(masks)
    refuse(N, F, n_ranks, T, P)
    W, bits = words_for(N), (1 << N) - 1
    masks = masks.reshape(F, W)
    C_ = case_words if isinstance(case_words, int) else to_int(case_words)
    if clean:
        C_ &= bits
    elif C_ >> N:
        raise Invalid("a case-mask bit at or above N")
    n1 = C_.bit_count()
    if n1 == 0 or n1 == N:
        raise Invalid("no case or no control")
    rank = np.asarray(table).reshape(-1).tolist()
    assert len(rank) == (N + 1) ** 2
    M = [to_int(row) for row in masks]
    w = [int(x) for x in np.asarray(mults).reshape(-1)]
    assert len(w) == F
    if clean:
        M = [x & bits for x in M]
    else:
        for m in range(N + 1):
            if any(rank[m * (N + 1) + k] >= n_ranks for k in au.feasible(N, n1, m)):
                raise Invalid("a feasible cell at or above n_ranks")
        if any(x >> N for x in M):
            raise Invalid("a mask with a bit at or above N")
        if sum(w) >= MAX_WEIGHT:
            raise Unsupported("multiplicity sum")
    row = [x.bit_count() * (N + 1) for x in M]
    obs = [rank[row[f] + (M[f] & C_).bit_count()] for f in range(F)]
    L = labels(int(seed), P, N, n1)
    least, tail = [n_ranks] * P, [0] * T
    part = [(M[f], row[f], w[f]) for f in range(F) if w[f]]
    for p, Lp in enumerate(L):
        lo = n_ranks
        for Mf, rf, wf in part:
            r = rank[rf + (Mf & Lp).bit_count()]
            if r < lo:
                lo = r
            if r < T:
                tail[r] += wf
        least[p] = lo
    stats = {"features": F, "features_weighted": len(part), "weight": sum(w), "permutations": P, "tail_total": sum(tail),
             "min_perm_rank": min(least) if P else n_ranks}
    return {"obs_rank": np.array(obs, dtype=np.uint32), "labels": rows_of(L, W), "perm_min": np.array(least, dtype=np.uint32),
            "tail": np.array(tail, dtype=np.uint64), "stats": stats}


def assert_same(got: dict, want: dict, what=""):
    for key in OUTPUTS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if key == "labels":
            assert len(g) == len(w), (what, key, g.shape, w.shape)
            g, w = g.reshape(-1), w.reshape(-1)      # (P x W, or P words where W is 1)
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        assert np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, key, np.argwhere(g.astype(np.uint64) != w.astype(np.uint64))[:8])


def python_permute_wide(calls=None):
    """The stand-in for nat.assoc_permute_wide: the contract, with a record of the calls."""
    def run(*args):
        if calls is not None:
            calls.append(args)
        return expected_permute_wide(*args)
    return run


# ---- tables ----

@functools.lru_cache(maxsize=32)
def census_table(N: int, n1: int):
    """A uint32 table in which every feasible cell has a rank of its own, numbered m ascending, k DEScending (it descends in k:
    not monotone the way a one-sided test is): with tail_ranks = n_ranks the tail is the (m, k) census.  (table, n_ranks)."""
    table = np.full((N + 1) * (N + 1), NO_RANK, dtype=np.uint32)
    n = 0
    for m in range(N + 1):
        ks = au.feasible(N, n1, m)
        table[m * (N + 1) + ks.start:m * (N + 1) + ks.stop] = np.arange(n + len(ks) - 1, n - 1, -1, dtype=np.uint32)
        n += len(ks)
    table.setflags(write=False)
    return table, n


@functools.lru_cache(maxsize=32)
def exact_table(N: int, n1: int, alternative: str):
    """(table uint32, n_ranks, tail_ranks at 1/20) of an exact test, from assoc_util.fisher_table: small N only (it is cubic)."""
    cells = au.fisher_table(N, n1, alternative)
    p_of_rank = sorted(set(cells.values()))
    rank_of = {p: r for r, p in enumerate(p_of_rank)}
    table = np.full((N + 1) * (N + 1), NO_RANK, dtype=np.uint32)
    for (m, k), p in cells.items():
        table[m * (N + 1) + k] = rank_of[p]
    table.setflags(write=False)
    return table, len(p_of_rank), sum(p * 20 <= 1 for p in p_of_rank)


def table_for(kind: str, N: int, n1: int):
    if kind == "census":
        table, n = census_table(N, n1)
        return table, n, n
    return exact_table(N, n1, kind)


# ---- the host build (tests/host_assoc_wide) ----

_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", HOST_DIR])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        for name in ("lanes", "slice", "max_samples", "max_permutations"):
            getattr(_host, "assoc_wide_host_" + name).restype = u32
        for name in ("words_for", "perms_per_lane", "block_perms"):
            getattr(_host, "assoc_wide_host_" + name).restype, getattr(_host, "assoc_wide_host_" + name).argtypes = u32, [u32]
        _host.assoc_wide_host_word_bits.restype, _host.assoc_wide_host_word_bits.argtypes = u64, [u32, u32]
        _host.assoc_wide_host_select_labels.restype, _host.assoc_wide_host_select_labels.argtypes = None, [u64, u32, u32, u32, vp]
        _host.assoc_wide_host_refuse.restype, _host.assoc_wide_host_refuse.argtypes = C.c_int, [u32, u64, u32, u32, u32]
        _host.assoc_wide_host_refuse_cases.restype, _host.assoc_wide_host_refuse_cases.argtypes = C.c_int, [u32, vp, C.c_int]
        _host.assoc_wide_host_permute.restype = C.c_int
        _host.assoc_wide_host_permute.argtypes = [u32, vp, u32, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, vp]
    return _host


def constant(name: str, *args) -> int:
    """LANES, SLICE, and per number of words PERMS_PER_LANE and BLOCK_PERMS, as the kernels have them."""
    return int(getattr(host_lib(), "assoc_wide_host_" + name.lower())(*args))


def host_permute(masks, mults, n_samples, case_words, table, n_ranks, tail_ranks, permutations, seed):
    """assoc_wide_host_permute — the primitive's steps on the host: (the four outputs, the blocks' flushes, their runs)."""
    N, P, T = int(n_samples), int(permutations), int(tail_ranks)
    W = words_for(N)
    mk, ml = np.ascontiguousarray(masks, np.uint64).reshape(-1, W), np.ascontiguousarray(mults, np.uint32)
    cw = to_words(case_words, W) if isinstance(case_words, int) else np.ascontiguousarray(case_words, np.uint64)
    tb = np.ascontiguousarray(table, np.uint32)
    F = len(mk)
    obs, labels_, least = np.zeros(max(F, 1), np.uint32), np.zeros((max(P, 1), W), np.uint64), np.zeros(max(P, 1), np.uint32)
    tail, counts = np.zeros(max(T, 1), np.uint64), np.zeros(2, np.uint64)
    rc = host_lib().assoc_wide_host_permute(N, cw.ctypes.data, F, mk.ctypes.data, ml.ctypes.data, tb.ctypes.data, int(n_ranks), T, P, int(seed),
                                            obs.ctypes.data, labels_.ctypes.data, least.ctypes.data, tail.ctypes.data, counts.ctypes.data)
    assert rc == 0, rc
    return {"obs_rank": obs[:F], "labels": labels_[:P], "perm_min": least[:P], "tail": tail[:T]}, int(counts[0]), int(counts[1])


# ---- constructed cases: name -> the arguments of the contract (masks[F, W], mults, N, case words, table, n_ranks, tail_ranks, P, seed)

def seeded_rows(N: int, F: int, seed: int, order="shuffled") -> np.ndarray:
    """F presence patterns of N samples as F x W words: most features in 2 to 4 samples, every seventh in about an eighth of
    them, every tenth in about half; `order`: shuffled (as drawn: nearly every feature starts a run of its own popcount) or
    ascending (by popcount, stable)."""
    rng = np.random.default_rng(seed)
    W = words_for(N)
    ints = []
    for f in range(F):
        if f % 10 == 0:
            x = int.from_bytes(rng.bytes(8 * W), "little")
        elif f % 7 == 0:
            x = int.from_bytes(rng.bytes(8 * W), "little") & int.from_bytes(rng.bytes(8 * W), "little") & int.from_bytes(rng.bytes(8 * W), "little")
        else:
            x = sum(1 << int(s) for s in set(rng.integers(0, N, size=int(rng.integers(2, 5)))))
        ints.append(x & ((1 << N) - 1))
    if order == "ascending":
        ints.sort(key=lambda x: x.bit_count())
    return rows_of(ints, W)


def case(N, n1, F, P, kind="census", seed=1, mask_seed=3, order="shuffled", tail_ranks=None):
    C_ = au.half_cases(N, n1)
    table, n_ranks, tail = table_for(kind, N, C_.bit_count())
    rows, mults = seeded_rows(N, F, mask_seed), au.seeded_mults(F, mask_seed)
    if order == "ascending":      # the same features with the same multiplicities, by popcount (stable)
        by = sorted(range(F), key=lambda f: to_int(rows[f]).bit_count())
        rows, mults = rows[by], mults[by]
    return (rows, mults, N, to_words(C_, words_for(N)), table, n_ranks, tail if tail_ranks is None else tail_ranks, P, seed)


SAMPLE_COUNTS = (2, 63, 64, 65, 127, 128, 129, 255, 257, 511, 513, 1023, 1024)


@functools.lru_cache(maxsize=1)
def constructed() -> dict:
    SLICE = constant("slice")
    out = {}
    for N in SAMPLE_COUNTS:      # every word count's edge; census: every feasible cell a rank of its own, descending in k
        out[f"N{N}_census"] = case(N, None, 150, 70, "census", seed=N)
    for N in (65, 70):
        for kind in ("greater", "two-sided", "less"):
            out[f"N{N}_{kind}"] = case(N, 30, 257, 130, kind, seed=N)
    out["N1024_one_case"] = case(1024, 1, 120, 65, "census", seed=5)
    out["N1024_one_control"] = case(1024, 1023, 120, 65, "census", seed=6)
    out["N130_one_case"] = case(130, 1, 256, 255, "census", seed=5)
    out["N130_one_control"] = case(130, 129, 255, 256, "census", seed=6)
    for N in (100, 400, 900):      # 2, 7 and 15 words: four, two and one relabeling a lane
        B = constant("block_perms", words_for(N))
        for P in (B - 1, B, B + 1):
            out[f"N{N}_P{P}"] = case(N, None, 40, P, "census", seed=P)
    for F in (0, 1, SLICE - 1, SLICE, SLICE + 1):
        out[f"F{F}"] = case(100, 40, F, 33, "census", seed=F)
    for P in (0, 1):
        out[f"P{P}"] = case(100, 40, 40, P, "census", seed=P)
    out["past_both"] = case(70, 30, SLICE + 1, constant("block_perms", 2) + 1, "greater", seed=10)
    out["ascending_popcount"] = case(200, 90, 2 * SLICE + 5, 70, "census", seed=21, order="ascending")
    out["shuffled_popcount"] = case(200, 90, 2 * SLICE + 5, 70, "census", seed=21, order="shuffled")
    out["tail_0"] = case(100, 50, 100, 100, "census", seed=11, tail_ranks=0)
    out["tail_1"] = case(100, 50, 100, 100, "census", seed=12, tail_ranks=1)
    out["seed_0"] = case(130, 60, 100, 100, "census", seed=0)
    out["seed_max"] = case(130, 60, 100, 100, "census", seed=(1 << 64) - 1)
    # the census of a balanced cohort of 1024: 263 169 ranks, all of them in the tail; dense features of about 512 samples have
    # cells far above 65 535
    out["N1024_ranks_above_16_bits"] = case(1024, 512, 60, 40, "census", seed=31)
    # popcount 0 and N, the case mask itself, and masks whose only bits lie in the last, partial word
    masks, mults, N, cw, table, n_ranks, tail, P, seed = case(130, 60, 12, 130, "census", seed=14)
    masks = masks.copy()
    masks[0] = 0
    masks[1] = to_words((1 << 130) - 1, 3)
    masks[2] = cw
    masks[3] = to_words(0b11 << 128, 3)
    masks[4] = to_words(0b01 << 128, 3)
    masks[5] = to_words(0b10 << 128, 3)
    out["popcount_0_and_N_the_case_mask_the_last_word"] = (masks, np.arange(1, 13, dtype=np.uint32), N, cw, table, n_ranks, tail, P, seed)
    # multiplicities: 0 and 2^32 - 1, and three features of one mask that sum to 2^32 - 1 at P = 257: a tail cell passes 2^32
    masks, mults, N, cw, table, n_ranks, tail, P, seed = case(130, 60, 8, 257, "census", seed=13)
    out["one_full_multiplicity"] = (masks, np.array([0, (1 << 32) - 1, 0, 0, 0, 0, 0, 0], dtype=np.uint32), N, cw, table, n_ranks, tail, P, seed)
    masks = masks.copy()
    masks[2] = masks[5] = masks[7] = to_words((0x0F0F << 60) | 1, 3)
    out["three_of_one_mask_sum_to_2_32_less_1"] = (masks, np.array([0, 0, 1 << 31, 0, 0, (1 << 31) - 2, 0, 1], dtype=np.uint32), N, cw, table,
                                                   n_ranks, tail, P, seed)
    masks, mults, N, cw, table, n_ranks, tail, P, seed = case(130, 60, 300, 100, "census", seed=15)
    out["all_multiplicities_0"] = (masks, np.zeros(300, np.uint32), N, cw, table, n_ranks, tail, P, seed)
    # contention: every feature is the case mask itself, two slices of them and more than a block of relabelings
    N, C_ = 66, 0b111 << 63
    table, n_ranks, tail = table_for("greater", N, 3)
    out["every_feature_is_the_case_mask"] = (np.tile(to_words(C_, 2), (2 * SLICE + 3, 1)), np.full(2 * SLICE + 3, 3, dtype=np.uint32), N,
                                             to_words(C_, 2), table, n_ranks, max(tail, 1), 300, 14)
    return out


def constructed_names() -> list:
    return list(constructed())


def premise(name: str, args, want):
    """What a constructed case is for, checked on the contract's own result."""
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = args
    weight = int(np.asarray(mults, dtype=np.uint64).sum())
    if name.endswith("_census") or name.startswith(("F", "N1024_", "ascending", "shuffled")) or "_P" in name:
        assert tail_ranks == n_ranks and int(want["tail"].sum()) == weight * P      # every pair is in the census
    if name == "N1024_ranks_above_16_bits":
        assert n_ranks == 263169 and tail_ranks > 65536 and int(want["obs_rank"].max()) > 65535 and int(np.flatnonzero(want["tail"]).max()) > 65535
    if name in ("three_of_one_mask_sum_to_2_32_less_1", "one_full_multiplicity"):
        assert weight == (1 << 32) - 1 and int(want["tail"].max()) >= 1 << 32
    if name == "all_multiplicities_0":
        assert (want["perm_min"] == n_ranks).all() and not want["tail"].any()
    if name == "tail_0":
        assert len(want["tail"]) == 0
    if name in ("ascending_popcount", "shuffled_popcount"):
        m = [to_int(r).bit_count() for r in masks]
        assert (m == sorted(m)) == (name == "ascending_popcount")
    if name == "N70_two-sided":
        n1 = to_int(cw).bit_count()
        row = [int(table[20 * (N + 1) + k]) for k in au.feasible(N, n1, 20)]
        assert row != sorted(row) and row != sorted(row, reverse=True)      # not monotone in k


# ---- the hand-written cohort of the wide stage tests: 70 samples used (27 cases) in two tabulate.tsv files, 40 + 30; one more
# sample with group `.` in the first file and one more without a row in -ph in the second ----

FIRST = [f"A{i:02d}" for i in range(41)]       # the first run's samples, in column order
SECOND = [f"B{i:02d}" for i in range(31)]      # the second run's
UNKNOWN, NOT_IN_PH = "A17", "B09"
USED = [s for s in FIRST + SECOND if s not in (UNKNOWN, NOT_IN_PH)]
CASES = USED[1:40:3] + USED[40:54]             # 13 of the first file's 40, 14 of the second's 30: not a prefix of the columns
# name -> (the samples it is present in with (clonotypes, reads); everyone else has (0, 0))
FEATURES = [
    ("exactly_the_cases", {s: (2, 9) for s in CASES}),
    ("everywhere", {s: (1, 3) for s in FIRST + SECOND}),
    ("nowhere", {}),
    ("the_last_six", {s: (1, 1) for s in USED[64:]}),
    ("across_the_words", {s: (3, 4) for s in USED[60:68]}),
    ("one_mask_a", {CASES[0]: (1, 2), CASES[20]: (3, 4), USED[0]: (1, 1)}),
    ("one_mask_b", {CASES[0]: (5, 5), CASES[20]: (1, 7), USED[0]: (2, 2)}),
    ("mostly_controls", {s: (1, 2) for s in USED if s not in CASES} | {CASES[2]: (1, 1)}),
    ("most_cases", {s: (1, 1) for s in CASES[:22]} | {USED[0]: (1, 5)}),
    ("the_second_run_alone", {s: (2, 2) for s in SECOND}),
    ("one_read_somewhere", {CASES[3]: (1, 1), CASES[24]: (1, 2), USED[5]: (1, 1), UNKNOWN: (4, 4), NOT_IN_PH: (2, 6)}),
]
assert len(USED) == 70 and len(CASES) == 27


def phenotype_text() -> bytes:
    lines = ["donor\tsample\tage\tgroup"]
    for i, s in enumerate(FIRST + SECOND):
        if s == NOT_IN_PH:
            continue
        group = "." if s == UNKNOWN else ("CMV+" if s in CASES else "CMV-")
        lines.append(f"d{i}\t{s}\t{30 + i}\t{group}")
    return ("\n".join(lines) + "\n").encode()


def tabulate_text(samples) -> bytes:
    """The tabulate.tsv of one run over `samples` (FIRST, SECOND, or both for the same cohort as ONE table)."""
    head = ["metaclonotype", "v_call", "j_call", "junction_aa", "radius", "samples"] + [f"{s}_{w}" for s in samples for w in ("clonotypes", "reads")]
    lines = ["\t".join(head)]
    for n, (name, where) in enumerate(FEATURES):
        cells = [str(n * 3), f"TRBV{n + 2}*01", "TRBJ2-1*01", "CASS" + name.upper().replace("_", "") + "F", str(12 + 2 * n),
                 str(sum(1 for s in samples if s in where))]
        for s in samples:
            cells += [str(where.get(s, (0, 0))[0]), str(where.get(s, (0, 0))[1])]
        lines.append("\t".join(cells))
    return ("\n".join(lines) + "\n").encode()


def identity_rows():
    lines = tabulate_text(FIRST).split(b"\n")[:-1]
    return [h.decode() for h in lines[0].split(b"\t")[:5]], [b"\t".join(x.split(b"\t")[:5]) for x in lines[1:]]


def hand_masks(value="clonotypes", min_count=1) -> list:
    """The features' presence over USED (bit i: USED[i]) as integers — from FEATURES, not from the files."""
    at = 0 if value == "clonotypes" else 1
    return [sum(1 << i for i, s in enumerate(USED) if where.get(s, (0, 0))[at] >= min_count) for _, where in FEATURES]


HAND_CASE_MASK = sum(1 << i for i, s in enumerate(USED) if s in CASES)


def wide_cohort_texts(n_samples: int, files: int):
    """A plain cohort of n_samples samples (every third a case) over `files` tabulate.tsv of equal share, three features:
    (the tables' texts, the phenotype's text)."""
    names = [f"X{i:04d}" for i in range(n_samples)]
    share = (n_samples + files - 1) // files
    where = [set(names[::3]), set(names[: n_samples // 2]), set(names[5:9])]
    tables = []
    for a in range(0, n_samples, share):
        part = names[a:a + share]
        lines = ["\t".join(["metaclonotype", "v_call", "j_call", "junction_aa", "radius", "samples"] + [f"{s}_{w}" for s in part for w in ("clonotypes", "reads")])]
        for n, have in enumerate(where):
            lines.append("\t".join([str(n), "TRBV9*01", "TRBJ2-7*01", f"CASSQ{'G' * n}F", "12", str(sum(s in have for s in part))]
                                   + [x for s in part for x in (("1", "2") if s in have else ("0", "0"))]))
        tables.append(("\n".join(lines) + "\n").encode())
    ph = "sample\tgroup\n" + "".join(f"{s}\t{'CMV+' if i % 3 == 0 else 'CMV-'}\n" for i, s in enumerate(names))
    return tables, ph.encode(), names, where
