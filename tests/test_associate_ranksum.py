"""`associate --test rank-sum` without a GPU: the scores against a brute-force mid-rank and z against scipy's asymptotic
Mann-Whitney; the bounds of the fixed-point score; the contract (tests/assoc_ranksum_util.expected_ranksum) against an enumeration
in Python integers; the host build of the shared code and of the primitive's steps against the contract on every constructed
case; the stand-alone program; exports and ABI; every refusal of both entries, in order, and the calls answered on the host; the
stage with the native call replaced by the contract against files written from their definitions, its refusals and its help; and
the default test's bytes, unchanged."""
import builtins
import gzip
import os
import re
import subprocess
from fractions import Fraction
from math import isqrt

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import associate as asc
from tests import assoc_ranksum_util as ru
from tests import assoc_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
U32 = (1 << 32) - 1


# ---- the scores ----

def _values(rng, F, N, top):
    return rng.integers(0, top, size=(F, N), dtype=np.int64)


@pytest.mark.parametrize("N,top", [(2, 3), (5, 2), (16, 4), (33, 1000), (64, 3), (64, 10 ** 9)])
def test_rank_scores_against_a_brute_force_mid_rank(N, top):
    rng = np.random.default_rng(N * 7 + top)
    x = _values(rng, 40, N + 3, top)
    used = [i for i in range(N + 3) if i not in (1, N)][:N]      # not a prefix of the columns
    for min_count in (1, 2):
        a = asc.rank_scores(x, used, min_count)
        assert a.shape == (40, N) and a.dtype == np.int64
        for f in range(40):
            cut = [int(v) if v >= min_count else 0 for v in x[f, used]]
            assert a[f].tolist() == ru.mid_rank_scores(cut), (f, cut)
        assert int(a.min()) == 0 and int(a.max()) <= 2 * N - 2


def test_rank_scores_on_the_edges():
    assert asc.rank_scores(np.full((2, 9), 4), range(9), 1).tolist() == [[0] * 9] * 2      # all equal: Q = 0
    a = asc.rank_scores(np.arange(64)[None, ::-1].copy(), range(64), 1)
    assert sorted(a[0].tolist()) == list(range(0, 127, 2)) and a[0, 0] == 126      # all distinct: a reaches 2 N - 2
    one = np.zeros((1, 64), dtype=np.int64)
    one[0, 17] = 5
    a = asc.rank_scores(one, range(64), 1)
    assert a[0, 17] == 64 and int(a.sum()) == 64      # one non-zero sample: d = 64 for the 63 zeros, 128 for it
    assert asc.rank_scores(one, range(64), 6).tolist() == [[0] * 64]      # below --min-count it counts as 0
    assert asc.rank_scores(np.array([[3, 1], [2, 2], [0, 9]]), range(2), 1).tolist() == [[2, 0], [0, 0], [0, 2]]      # N = 2
    assert asc.rank_scores(np.zeros((0, 5), dtype=np.int64), range(5), 1).shape == (0, 5)
    for a in (asc.rank_scores(np.full((2, 9), 4), range(9), 1), asc.rank_scores(one, range(64), 1)):
        planes, off, sc = asc.ranksum_inputs(a, 3)
        want = ru.inputs_of(a.tolist(), 3)
        assert np.array_equal(planes, want[0]) and np.array_equal(off, want[1]) and np.array_equal(sc, want[2])
    assert asc.ranksum_inputs(np.zeros((3, 9), np.int64), 4)[2].tolist() == [0, 0, 0]      # Q = 0: scale 0


def test_rank_scores_with_depths():
    x = np.array([[10, 3, 0, 5], [1, 1, 1, 1], [0, 0, 0, 0]])
    depths = [1000, 100, 50, 1000]      # 10/1000 < 3/100: the raw order of samples 0 and 1 is reversed
    raw, deep = asc.rank_scores(x, range(4), 1), asc.rank_scores(x, range(4), 1, depths)
    assert raw[0, 0] > raw[0, 1] and deep[0, 0] < deep[0, 1]
    for f in range(3):
        assert deep[f].tolist() == ru.mid_rank_scores(x[f].tolist(), depths)
    assert deep[1].tolist() == ru.mid_rank_scores([1, 1, 1, 1], depths) and len(set(deep[1].tolist())) == 3      # equal values, unequal depths
    big = np.array([[3 * 10 ** 17, 10 ** 17 + 1]])      # products past 2^64: Python integers
    assert asc.rank_scores(big, range(2), 1, [3 * 10 ** 17 - 1, 10 ** 17]).tolist() == [ru.mid_rank_scores([3 * 10 ** 17, 10 ** 17 + 1], [3 * 10 ** 17 - 1, 10 ** 17])]
    with pytest.raises(ValueError) as e:
        asc.rank_scores(x, range(4), 1, [1000, 0, 50, 1000], names=["A", "B", "C", "D"])
    assert "'B'" in str(e.value) and "depth of 0" in str(e.value)
    assert asc.rank_scores(x[[0, 2]], range(4), 1, [1000, 100, 0, 1000]).tolist() == deep[[0, 2]].tolist()      # a depth of 0 under values of 0 is no error
    assert asc.rank_scores(x, range(4), 4, [1000, 0, 50, 1000])[0].tolist() == ru.mid_rank_scores([10, 0, 0, 5], [1000, 1, 50, 1000])      # cut first


# ---- z against scipy ----

@pytest.mark.parametrize("N,n1", [(64, 32), (64, 20), (16, 8), (5, 2)])
@pytest.mark.parametrize("ties", [False, True])
def test_z_against_scipys_asymptotic_mann_whitney(N, n1, ties):
    """The tolerance is a relative 1e-12: a guard on double rounding, not a measurement (4e-15 was seen)."""
    from scipy import stats
    rng = np.random.default_rng(N * 100 + n1 + ties)
    C_ = au.half_cases(N, n1)
    in_cases = np.array([bool(C_ >> s & 1) for s in range(N)])
    for trial in range(20):
        x = rng.integers(0, 4, size=N) if ties else rng.permutation(N * 3)[:N]
        if len(set(x.tolist())) == 1:
            continue
        a = asc.rank_scores(x[None, :], range(N), 0)[0]
        A, B, Q, offset, scale = ru.sums(a.tolist(), n1)
        D = int(asc.ranksum_D(a[None, :], C_, n1)[0])
        assert D == N * int(a[in_cases].sum()) - offset
        z = ru.z_of(D, Q, N, n1)
        for alternative in ("greater", "less", "two-sided"):
            res = stats.mannwhitneyu(x[in_cases], x[~in_cases], alternative=alternative, method="asymptotic", use_continuity=False)
            p = {"greater": stats.norm.sf(z), "less": stats.norm.cdf(z), "two-sided": 2 * stats.norm.sf(abs(z))}[alternative]
            assert abs(p - res.pvalue) <= 1e-12 * max(res.pvalue, 1e-300) or abs(p - res.pvalue) < 1e-300, (alternative, p, res.pvalue)
        U = res.statistic if alternative != "less" else res.statistic      # scipy's statistic is the cases' U whatever the alternative
        mean, var_z = n1 * (N - n1) / 2, None
        assert abs((U - mean) - D / (2 * N)) <= 1e-9      # D = 2 N (U - n1 n0 / 2)
        assert format(z, ".6g") == asc.z_text(D, Q, N, n1)
    assert asc.z_text(0, 0, N, n1) == "nan"


def test_the_bounds_of_the_fixed_point_score():
    worst_t = worst_u = 0
    for N in range(2, 65):
        for n1 in sorted({1, N // 2, N - 1}):
            extremes = [list(range(N)), [0] * (N - 1) + [1], [0] + [1] * (N - 1), [0] * (N - n1) + [1] * n1, [s // 2 for s in range(N)]]
            for x in extremes:
                a = ru.mid_rank_scores(x)
                A, B, Q, offset, scale = ru.sums(a, n1)
                assert (Q == 0) == (len(set(x)) == 1) == (scale == 0)      # Q = 0 exactly when all values are equal
                if Q == 0:
                    continue
                assert max(a) <= 2 * N - 2 <= 126 and 4 <= Q < 1 << 23 and offset <= U32 and scale <= U32
                top = sorted(a, reverse=True)
                for W in (sum(top[:n1]), sum(top[-n1:])):      # the extreme labelings
                    D = N * W - offset
                    assert abs(D) <= n1 * (N - n1) * (2 * N - 2) < 1 << 20      # D is a sum over (case, control) pairs of a difference of scores
                    for alt in (0, 1, 2):
                        t = ru.score(D, scale, alt)
                        assert t == asc.ranksum_score(D, scale, ru.ALTERNATIVES[alt])
                        worst_t, worst_u = max(worst_t, t), max(worst_u, abs(D))
    assert worst_t < 1 << 32 and worst_u < 1 << 20 and worst_u == 64 * 32 * 32      # all distinct at N = 64, the top half the cases
    assert ru.score(1 << 40, U32, 0) == (((1 << 20) - 1) * U32) >> 20 < U32      # the clamp: t < 2^32 whatever the arrays hold
    assert ru.score(-(1 << 40), U32, 0) == 0 and ru.score(-(1 << 40), U32, 1) == ru.score(1 << 40, U32, 2)
    assert min(U32, isqrt((1 << 64) // 4)) == 1 << 31      # the largest scale a real feature has (Q = 4 at N = 2)


# ---- the contract against an enumeration ----

@pytest.mark.parametrize("N,n1,alt", [(2, 1, 0), (3, 1, 2), (5, 2, 1), (8, 4, 2), (8, 3, 0), (7, 6, 1)])
def test_the_contract_against_an_enumeration_in_python_integers(N, n1, alt):
    rng = np.random.default_rng(N * 10 + alt)
    x = rng.integers(0, 3, size=(12, N))
    x[3] = 1
    scores = [ru.mid_rank_scores(row.tolist()) for row in x]
    planes, off, sc = ru.inputs_of(scores, n1)
    mults = np.array([1, 2, 0, 4, 5, 0, 7, 8, 9, 1, 1, 3], np.uint32)
    C_ = au.half_cases(N, n1)
    edges = ru.top_edges(planes, off, sc, N, C_, alt, 5)
    want = ru.enumerated(scores, off, sc, mults, N, C_, alt, [int(e) for e in edges], 40, 9)
    got = ru.expected_ranksum(planes, off, sc, mults, N, C_, alt, edges, 40, 9)
    for key in ("obs_score", "perm_max", "exceed", "tail"):
        assert [int(v) for v in got[key]] == want[key], key
    assert [int(v) for v in got["labels"]] == [au.labels(9, p, N, n1) for p in range(40)]
    assert got["stats"]["tail_total"] == sum(want["tail"]) and got["stats"]["max_perm_score"] == max(want["perm_max"])


# ---- the host build ----

def test_host_constants_and_shared_functions():
    H = ru.host_lib()
    assert [ru.constant(k) for k in ("lanes", "perms_per_lane", "block_perms", "slice", "planes", "shift", "max_edges")] == [256, 4, 1024, 1024, 7, 20, 1024]
    assert ru.constant("slice") % ru.constant("group") == 0
    rng = np.random.default_rng(2)
    for _ in range(200):
        a = rng.integers(0, 127, size=64).tolist()
        L = int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2))
        pl = np.array(ru.planes_of(a), np.uint64)
        W = H.assoc_ranksum_host_weighted_sum(pl.ctypes.data, L)
        assert W == sum(v for s, v in enumerate(a) if L >> s & 1)
        off, sc = int(rng.integers(0, 1 << 32)) if _ % 4 == 0 else int(rng.integers(0, 1 << 19)), int(rng.integers(0, 1 << 32))
        for alt in (0, 1, 2):
            assert H.assoc_ranksum_host_score_of(W, 64, off, sc, alt) == ru.score(64 * W - off, sc, alt)
    edges = np.array([3, 4, 10, 1 << 31, U32 - 1], np.uint32)
    for t, want in ((0, U32), (2, U32), (3, 0), (9, 1), (10, 2), ((1 << 31) - 1, 2), (1 << 31, 3), (U32 - 1, 4), (U32, 4)):
        assert H.assoc_ranksum_host_edge_of(edges.ctypes.data, 5, t) == want
    assert H.assoc_ranksum_host_edge_of(edges.ctypes.data, 0, 7) == U32
    dirty = np.array([9, 1, 9, 1, 9, 1, 9], np.uint32)      # not ascending: some cell inside, or none
    assert all(H.assoc_ranksum_host_edge_of(dirty.ctypes.data, 7, t) in list(range(7)) + [U32] for t in range(12))


@pytest.mark.parametrize("name", ru.constructed_names())
def test_host_build_against_the_contract(name):
    args = ru.constructed()[name]
    want = ru.expected_ranksum(*args)
    ru.premise(name, args, want)
    got, counts = ru.host_run(*args)
    ru.assert_same(got, want, name)
    F, P, E = len(args[0]), args[8], len(args[7])
    waves = ru.constant("lanes") // 64
    tiles, slices = -(-P // ru.constant("block_perms")), -(-F // ru.constant("slice"))
    assert counts[0] <= F * tiles * waves and counts[1] <= F * tiles and counts[2] <= E * tiles * slices      # one add per (wave, feature) at most


def test_the_stand_alone_program_runs_plain():
    ru.host_lib()
    out = subprocess.run([ru.HOST_MAIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok") and ": 0 differ" in out.stdout and "FAILED" not in out.stdout
    makefile = open(os.path.join(ru.HOST_DIR, "Makefile")).read()
    assert "asan:" in makefile and "-fsanitize=address,undefined" in makefile and "assoc_ranksum_main_asan" in makefile


# ---- exports and ABI ----

def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "#define DCRX_ABI_VERSION 5" in hdr and nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    for name in ("dcrx_assoc_ranksum_device", "dcrx_assoc_ranksum"):
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(nat.lib(), name)
    assert "#define DCRX_ASSOC_RANKSUM_PLANES 7" in hdr and nat.ASSOC_RANKSUM_PLANES == 7
    assert "#define DCRX_ASSOC_RANKSUM_SHIFT 20" in hdr and nat.ASSOC_RANKSUM_SHIFT == 20
    assert "#define DCRX_ASSOC_RANKSUM_MAX_EDGES 1024" in hdr and nat.ASSOC_RANKSUM_MAX_EDGES == 1024
    assert nat.ASSOC_RANKSUM_STATS == ru.STATS
    assert "#define DCRX_ASSOC_MAX_SAMPLES 64" in hdr and "#define DCRX_ASSOC_WIDE_MAX_SAMPLES 1024" in hdr      # the other layers stay
    section = flat[flat.index("---- association, rank-sum"):flat.index("---- the CDR3 network, weighted")]
    for words in ("THE ENTRY TAKES NO WORK SPACE", "in this order", "strictly ascending", "ANDs every plane", "clamps u", "inside 0 .. E - 1",
                  "for EVERY feature", "falls in no cell", "the words dcrx_assoc_permute returns", "F == 0 or P == 0"):
        assert words in section, words
    assert flat.count("THE ENTRY TAKES NO WORK SPACE") >= 3
    assert callable(nat.assoc_ranksum) and callable(nat.assoc_ranksum_device)
    makefile = open(os.path.join(ROOT, "decombinator_amd", "csrc", "Makefile")).read()
    assert "dcrx_assoc_ranksum.hip" in makefile and "dcrx_assoc_wide.hip" in makefile and "dcrx_assoc.hip" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"tests", "host_assoc_ranksum"' in entry
    core = open(os.path.join(ROOT, "decombinator_amd", "csrc", "dcrx_assoc_ranksum_core.h")).read()
    assert '#include "dcrx_assoc_core.h"' in core and "cannot wrap" in core and "u scale fits 64 bits" in core
    kernels = open(os.path.join(ROOT, "decombinator_amd", "csrc", "dcrx_assoc_ranksum.hip")).read()
    assert "stage_keys(" in kernels and "labels_from_keys(" in kernels and "key_of" not in kernels      # the selection is shared, not copied


def test_declared_equals_exported_still_holds():
    from tests import test_cabi
    checks = [getattr(test_cabi, n) for n in dir(test_cabi) if n.startswith("test_") and "export" in n.lower() or n.startswith("test_") and "declared" in n.lower()]
    assert checks
    for check in checks:
        if check.__code__.co_argcount == 0:
            check()


# ---- the refusals of both entries: on the host, before any device call, in the header's order ----

def _ok():
    return {"N": 16, "C": 0xFF, "alt": 0, "F": 2, "E": 3, "P": 5, "seed": 1}


def _both(a, pointers=None):
    """(code, message) of the host entry and of the device entry on the same scalars, with addresses that must not be looked
    behind before the refusal (pointers: plane, offset, scale, mult, edges, obs_score, labels, perm_max, exceed, tail)."""
    L = nat.lib()
    p = [0x1000] * 10 if pointers is None else pointers
    out = []
    for entry in (L.dcrx_assoc_ranksum, L.dcrx_assoc_ranksum_device):
        rc = entry(a["N"], a["C"], a["alt"], a["F"], p[0], p[1], p[2], p[3], a["E"], p[4], a["P"], a["seed"], p[5], p[6], p[7], p[8], p[9], None)
        out.append((rc, L.dcrx_last_error().decode()))
    return out


SCALAR_REFUSALS = [
    ({"N": 1, "C": 1}, E_INVALID, "samples"), ({"N": 65}, E_INVALID, "samples"), ({"N": 0}, E_INVALID, "samples"),
    ({"C": 1 << 16}, E_INVALID, "bit at or above"), ({"C": 0}, E_INVALID, "1 .. N - 1 cases"), ({"C": 0xFFFF}, E_INVALID, "1 .. N - 1 cases"),
    ({"alt": 3}, E_INVALID, "alternative"), ({"alt": U32}, E_INVALID, "alternative"), ({"E": 1025}, E_INVALID, "edges"),
    ({"F": 1 << 30}, E_UNSUPPORTED, "2^30"), ({"P": (1 << 20) + 1}, E_UNSUPPORTED, "permutations"),
    # the order: samples, case mask, alternative, edges, features, permutations
    ({"N": 65, "C": 0, "alt": 3, "E": 1025, "F": 1 << 30}, E_INVALID, "samples"), ({"C": 0, "alt": 3, "E": 1025}, E_INVALID, "1 .. N - 1 cases"),
    ({"alt": 3, "E": 1025, "F": 1 << 30}, E_INVALID, "alternative"), ({"E": 1025, "F": 1 << 30, "P": (1 << 20) + 1}, E_INVALID, "edges"),
    ({"F": 1 << 30, "P": (1 << 20) + 1}, E_UNSUPPORTED, "2^30"),
]


@pytest.mark.parametrize("change,code,word", SCALAR_REFUSALS)
def test_both_entries_refuse_the_scalars_first(change, code, word):
    for entry, (rc, msg) in zip(("dcrx_assoc_ranksum:", "dcrx_assoc_ranksum_device:"), _both(dict(_ok(), **change), pointers=[None] * 10)):
        assert rc == code and word in msg and entry in msg, (rc, msg)      # (null arrays too: the scalars come first)


def test_both_entries_refuse_null_arrays_next():
    a = _ok()
    for missing in range(10):
        p = [0x1000] * 10
        p[missing] = None
        for rc, msg in _both(a, pointers=p):
            assert rc == E_INVALID and "null argument" in msg, (missing, msg)
    # an array of no entries may be null: with no feature, no edge and no permutation the host entry answers
    L = nat.lib()
    assert L.dcrx_assoc_ranksum(16, 0xFF, 0, 0, None, None, None, None, 0, None, 0, 1, None, None, None, None, None, None) == 0
    assert L.dcrx_assoc_ranksum_device(16, 0xFF, 0, 0, None, None, None, None, 0, None, 0, 1, None, None, None, None, None, None) == 0


def _host_ok():
    scores = [ru.mid_rank_scores([0, 1, 2, 3, 0, 0, 0, 5, 1, 1, 1, 0, 0, 0, 2, 2]), ru.mid_rank_scores([0] * 15 + [1])]
    planes, off, sc = ru.inputs_of(scores, 8)
    return {"planes": planes, "offsets": off, "scales": sc, "mults": np.array([1, 2], np.uint32), "n_samples": 16, "case_mask": 0xFF,
            "alternative": "greater", "edges": np.array([1, 5, 9], np.uint32), "permutations": 5, "seed": 1}


def test_the_host_entry_refuses_what_it_sees_in_the_arrays_in_order():
    a = _host_ok()
    bad_planes = a["planes"].copy()
    bad_planes[1, 6] |= np.uint64(1 << 16)
    bad_edges = np.array([1, 5, 5], np.uint32)
    heavy = np.array([U32, 1], np.uint32)
    with pytest.raises(nat.DcrxError) as e:      # the planes before the edges and the multiplicities
        nat.assoc_ranksum(**dict(a, planes=bad_planes, edges=bad_edges, mults=heavy))
    assert e.value.code == E_INVALID and "plane has a bit at or above" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_ranksum(**dict(a, edges=bad_edges, mults=heavy))
    assert e.value.code == E_INVALID and "strictly ascending" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_ranksum(**dict(a, edges=np.array([5, 1, 9], np.uint32)))
    assert e.value.code == E_INVALID and "strictly ascending" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_ranksum(**dict(a, mults=heavy))
    assert e.value.code == E_UNSUPPORTED and "2^32" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:      # the scalars before all of them
        nat.assoc_ranksum(**dict(a, alternative=3, planes=bad_planes))
    assert e.value.code == E_INVALID and "alternative" in str(e.value)
    for change, word in (({"planes": a["planes"][:, :6]}, "planes are"), ({"mults": np.array([1], np.uint32)}, "multiplicity per feature"),
                         ({"scales": np.array([1, 1 << 32])}, "scale does not fit"), ({"alternative": "both"}, "alternative"),
                         ({"edges": np.array([-1, 2])}, "edges"), ({"seed": 1 << 64}, "seed")):
        with pytest.raises(ValueError) as e:
            nat.assoc_ranksum(**dict(a, **change))
        assert word in str(e.value), str(e.value)


def test_no_features_and_no_permutations_are_answered_on_the_host():
    a = _host_ok()
    got = nat.assoc_ranksum(**dict(a, permutations=0))
    want = ru.expected_ranksum(a["planes"], a["offsets"], a["scales"], a["mults"], 16, 0xFF, 0, a["edges"], 0, 1)
    ru.assert_same(got, want)
    assert got["stats"] == want["stats"] and len(got["obs_score"]) == 2 and got["obs_score"].any() and not got["tail"].any() and len(got["tail"]) == 3
    none = dict(a, planes=np.zeros((0, 7), np.uint64), offsets=np.zeros(0, np.uint32), scales=np.zeros(0, np.uint32), mults=np.zeros(0, np.uint32))
    got = nat.assoc_ranksum(**none)
    want = ru.expected_ranksum(none["planes"], none["offsets"], none["scales"], none["mults"], 16, 0xFF, 0, a["edges"], 5, 1)
    ru.assert_same(got, want)
    assert got["stats"] == want["stats"] and [int(x) for x in got["labels"]] == [au.labels(1, p, 16, 8) for p in range(5)] and not got["perm_max"].any()
    for alternative in (0, 1, 2, "less", "two-sided"):
        got = nat.assoc_ranksum(**dict(a, permutations=0, alternative=alternative))
        ru.assert_same(got, ru.expected_ranksum(a["planes"], a["offsets"], a["scales"], a["mults"], 16, 0xFF, alternative, a["edges"], 0, 1))


# ---- the stage over the contract ----

def _write(tmp_path, kind="tabulate", gz=False):
    text = ru.tabulate_text() if kind == "tabulate" else ru.public_text()
    name = ("dcr_tabulate.tsv" if kind == "tabulate" else "dcr_overlap_public.tsv") + (".gz" if gz else "")
    path = tmp_path / name
    path.write_bytes(gzip.compress(text) if gz else text)
    (tmp_path / "cohort.tsv").write_bytes(au.phenotype_text())
    (tmp_path / "dcr_tabulate_samples.tsv").write_bytes(ru.samples_text())
    return str(path), str(tmp_path / "cohort.tsv")


def _inp(tmp_path, infile, ph, **more):
    inp = {"command": "associate", "infile": infile, "phenotype": ph, "case": "CMV+", "outpath": str(tmp_path) + os.sep, "prefix": "t_",
           "dontgzip": True, "permutations": 99, "write_null": True, "test": "rank-sum"}
    inp.update(more)
    return inp


def _run(monkeypatch, inp):
    calls = []
    monkeypatch.setattr(nat, "assoc_ranksum", ru.python_ranksum(calls))
    return asc.run(inp), calls


def _read(name):
    return gzip.open(name, "rb").read() if name.endswith(".gz") else open(name, "rb").read()


@pytest.mark.parametrize("kind,value,min_count,alternative,depths,gz", [
    ("tabulate", None, 1, None, False, False), ("tabulate", None, 1, "less", False, False), ("tabulate", None, 1, "two-sided", False, False),
    ("tabulate", "reads", 2, None, False, False), ("tabulate", "clonotypes", 1, "greater", True, False), ("tabulate", "reads", 1, "two-sided", True, True),
    ("public", None, 1, "greater", False, True), ("public", "reads", 2, "less", False, False)])
def test_stage_writes_the_contracts_files(tmp_path, monkeypatch, capsys, kind, value, min_count, alternative, depths, gz):
    infile, ph = _write(tmp_path, kind, gz)
    inp = _inp(tmp_path, infile, ph, value=value, min_count=min_count if min_count != 1 else None, alternative=alternative, dontgzip=not gz,
               depths=str(tmp_path / "dcr_tabulate_samples.tsv") if depths else None)
    out, calls = _run(monkeypatch, inp)
    printed = capsys.readouterr().out
    assert len(calls) == 1      # ONE native call
    planes, off, sc, mults, N, case_mask, alt_given, edges, P, seed = calls[0]
    what = value or ("clonotypes" if kind == "tabulate" else "reads")
    alt = alternative or "greater"
    x_rows = ru.hand_values(what, min_count)
    deep = ru.hand_depths(what) if depths else None
    assert (N, case_mask, alt_given, P, seed) == (16, au.HAND_CASE_MASK, alt, 99, 1)
    hand_planes, hand_off, hand_sc = ru.inputs_of([ru.mid_rank_scores(x, deep) for x in x_rows], 8)
    distinct, first, counts = np.unique(hand_planes, axis=0, return_index=True, return_counts=True)
    assert np.array_equal(planes, distinct) and np.array_equal(mults, counts) and np.array_equal(off, hand_off[first]) and np.array_equal(sc, hand_sc[first])
    assert 2 in counts      # the two features of identical scores but different values
    null = ru.hand_null(x_rows, alt, 99, 1, deep)
    identity, rows = ru.identity_rows(kind)
    want_main, want_null, feats, want_edges = ru.stage_files(identity, rows, x_rows, 16, au.HAND_CASE_MASK, alt, 99, null, deep)
    assert [int(e) for e in edges] == want_edges      # the largest distinct observed scores, ascending
    assert out["associate"].endswith("t_associate.tsv" + (".gz" if gz else "")) and out["null"].endswith("t_associate_null.tsv" + (".gz" if gz else ""))
    assert _read(out["associate"]) == want_main      # byte for byte
    assert _read(out["null"]) == want_null
    lines = want_main.split(b"\n")
    assert lines[0].endswith(b"\tnonzero\tnonzero_cases\tnonzero_controls\tcases\tcontrols\tmean_rank_cases\tmean_rank_controls\tz\tscore\tp_value\tp_adjusted\tq_value")
    if alt == "greater" and not depths:
        assert lines[1].startswith(rows[0]) and b"\t12.5\t4.5\t" in lines[1]      # separates completely: the cases hold ranks 9 .. 16
    nan = [x for x in lines[1:-1] if b"\tnan\t0\t" in x]
    assert len(nan) == sum(1 for ft in feats if ft["Q"] == 0) >= (1 if depths else 2)      # constant and all-zero: Q = 0, score 0 (under depths the constant feature is none)
    assert f"Sample {au.NOT_IN_PH} of" in printed and "left out" in printed
    assert ("Ranking raw " + what in printed) == (not depths) and (f"over the depths of" in printed) == bool(depths)
    assert "16 samples used (8 cases, 8 controls; 1 left out without a group, 1 without a row in -ph)" in printed and "99 permutations, seed 1" in printed
    assert out["stats"]["features"] == len(x_rows) and out["stats"]["rows"] == len(distinct) and out["stats"]["test"] == "rank-sum"


def test_stage_without_permutations_makes_no_native_call(tmp_path, monkeypatch):
    infile, ph = _write(tmp_path)

    def boom(*a, **k):
        raise AssertionError("a native entry was called")
    for name in ("assoc_ranksum", "assoc_ranksum_device", "assoc_permute", "assoc_permute_wide", "lib", "check", "device_count"):
        monkeypatch.setattr(nat, name, boom)
    out = asc.run(_inp(tmp_path, infile, ph, permutations=0))
    identity, rows = ru.identity_rows("tabulate")
    want_main, want_null, _, _ = ru.stage_files(identity, rows, ru.hand_values("clonotypes", 1), 16, au.HAND_CASE_MASK, "greater", 0, None)
    assert open(out["associate"], "rb").read() == want_main and open(out["null"], "rb").read() == want_null
    body = want_main.split(b"\n")[1:-1]
    assert all(line.endswith(b"\t.\t.\t.") for line in body) and out["result"] is None
    assert all(line.split(b"\t")[-4].isdigit() and line.split(b"\t")[-5] != b"." for line in body)      # score and z are written


def test_stage_through_the_command_line(tmp_path, monkeypatch, capsys):
    from decombinator_amd import pipeline
    infile, ph = _write(tmp_path, gz=True)
    monkeypatch.setattr(nat, "assoc_ranksum", ru.python_ranksum())
    words = ["associate", "-in", infile, "-ph", ph, "--case", "CMV+", "-op", str(tmp_path) + os.sep, "--permutations", "50", "--seed", "3", "--test",
             "rank-sum", "--depths", str(tmp_path / "dcr_tabulate_samples.tsv"), "--value", "reads"]
    pipeline.main(words)
    assert "Associated 8 features" in capsys.readouterr().out
    a = _read(str(tmp_path / "dcr_associate.tsv.gz"))
    assert not (tmp_path / "dcr_associate_null.tsv.gz").exists()
    pipeline.main(words)
    assert _read(str(tmp_path / "dcr_associate.tsv.gz")) == a      # a second run gives the same bytes


def test_stage_refuses_65_used_samples_and_what_the_depths_hold(tmp_path, monkeypatch):
    monkeypatch.setattr(nat, "assoc_ranksum", ru.python_ranksum())
    names = [f"X{i:02d}" for i in range(65)]
    head = ["metaclonotype", "v_call", "j_call", "junction_aa", "radius", "samples"] + [f"{s}_{w}" for s in names for w in ("clonotypes", "reads")]
    (tmp_path / "wide.tsv").write_text("\t".join(head) + "\n" + "\t".join(["0", "TRBV2*01", "TRBJ2-1*01", "CASSF", "12", "65"] + ["1", "2"] * 65) + "\n")
    (tmp_path / "wide_cohort.tsv").write_text("sample\tgroup\n" + "".join(f"{s}\t{'a' if i % 2 else 'b'}\n" for i, s in enumerate(names)))
    with pytest.raises(ValueError) as e:
        asc.run(_inp(tmp_path, str(tmp_path / "wide.tsv"), str(tmp_path / "wide_cohort.tsv"), case="a"))
    assert "65" in str(e.value) and "64" in str(e.value) and "wide form" in str(e.value) and "not done" in str(e.value)
    infile, ph = _write(tmp_path)

    def fails(word, text):
        (tmp_path / "d.tsv").write_text(text)
        with pytest.raises(ValueError) as e:
            asc.run(_inp(tmp_path, infile, ph, depths=str(tmp_path / "d.tsv")))
        assert word in str(e.value), str(e.value)
    full = ru.samples_text().decode()
    fails("'S03'", "".join(line + "\n" for line in full.split("\n")[:-1] if not line.startswith("S03\t")))      # a used sample is missing
    fails("'S04'", full.replace("S04\t100\t", "S04\t0\t"))      # a depth of 0 under a non-zero value names the sample
    fails("no column 'clonotypes'", full.replace("\tclonotypes\t", "\tclones\t", 1))
    fails("no column 'sample'", full.replace("sample\t", "name\t", 1))
    fails("no count", full.replace("S04\t100\t", "S04\tmany\t"))
    fails("two rows", full + "S04\t1\t1\t1\t0\t0\t0\n")
    # a sample that is not used may be missing from --depths, and may have a depth of 0
    (tmp_path / "d.tsv").write_text("".join(line + "\n" for line in full.split("\n")[:-1] if not line.startswith(au.NOT_IN_PH + "\t")).replace(
        f"{au.UNKNOWN}\t1000\t", f"{au.UNKNOWN}\t0\t").replace(f"{au.UNKNOWN}\t100\t", f"{au.UNKNOWN}\t0\t"))
    asc.run(_inp(tmp_path, infile, ph, depths=str(tmp_path / "d.tsv"), permutations=0))


REFUSALS = [({"max_p": "0.05"}, "--max-p"), ({"max_p": "1"}, "--max-p"), ({"test": "fisher", "depths": "d.tsv"}, "--depths"),
            ({"test": None, "depths": "d.tsv"}, "--depths"), ({"test": "t"}, "--test"), ({"alternative": "both"}, "--alternative"),
            ({"permutations": (1 << 20) + 1}, "--permutations")]


@pytest.mark.parametrize("change,word", REFUSALS)
def test_stage_refuses_before_a_file_is_opened(tmp_path, monkeypatch, change, word):
    def no_open(*a, **k):
        raise AssertionError("a file was opened")
    inp = dict(_inp(tmp_path, str(tmp_path / "missing.tsv"), str(tmp_path / "missing_too.tsv")), **change)
    assert word in asc.refusal(inp)
    monkeypatch.setattr(builtins, "open", no_open)
    monkeypatch.setattr(gzip, "open", no_open)
    with pytest.raises(ValueError) as e:
        asc.run(inp)
    assert word in str(e.value)


def test_the_help_names_the_new_flags_and_keeps_its_sentences():
    from decombinator_amd.io import cli_args, create_associate_parser
    text = " ".join(create_associate_parser().format_help().split())
    for flag in ("--test", "--depths", "rank-sum", "fisher", "-in", "-ph", "--case", "--value", "--min-count", "--alternative", "--permutations", "--seed",
                 "--max-p", "--write-null"):
        assert flag in text, flag
    assert "design choices after Emerson et al., not measured optima" in text and "presence, not abundance" in text      # the default test's
    assert "tabulate_samples.tsv fits as it stands" in text and "max-T" in text and "2 to 64 samples" in text
    inp = cli_args(["associate", "-in", "a.tsv", "-ph", "c.tsv", "--case", "X", "--test", "rank-sum", "--depths", "d.tsv"])
    assert inp["test"] == "rank-sum" and inp["depths"] == "d.tsv" and inp["max_p"] is None
    inp = cli_args(["associate", "-in", "a.tsv", "-ph", "c.tsv", "--case", "X"])
    assert inp["test"] is None and inp["depths"] is None
    with pytest.raises(SystemExit):
        cli_args(["associate", "-in", "a.tsv", "-ph", "c.tsv", "--case", "X", "--test", "t-test"])
    assert "THE TEST IS ON PRESENCE, NOT ABUNDANCE" in asc.__doc__ and "--test rank-sum" in asc.__doc__


# ---- the default test writes what it wrote ----

@pytest.mark.parametrize("test", [None, "fisher"])
@pytest.mark.parametrize("kind,alternative", [("tabulate", None), ("public", "two-sided")])
def test_without_the_flag_the_bytes_are_the_presence_tests(tmp_path, monkeypatch, capsys, test, kind, alternative):
    text = au.tabulate_text() if kind == "tabulate" else au.public_text()
    (tmp_path / "in.tsv").write_bytes(text)
    (tmp_path / "cohort.tsv").write_bytes(au.phenotype_text())
    calls = []
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute(calls))

    def boom(*a, **k):
        raise AssertionError("the rank-sum entry was called")
    monkeypatch.setattr(nat, "assoc_ranksum", boom)
    inp = {"command": "associate", "infile": str(tmp_path / "in.tsv"), "phenotype": str(tmp_path / "cohort.tsv"), "case": "CMV+",
           "outpath": str(tmp_path) + os.sep, "prefix": "t_", "dontgzip": True, "permutations": 99, "write_null": True, "alternative": alternative}
    if test:
        inp["test"] = test
    out = asc.run(inp)
    printed = capsys.readouterr().out
    alt = alternative or "greater"
    hand = au.hand_masks("clonotypes" if kind == "tabulate" else "reads", 1)
    table, p_of_rank = au.rank_table(16, 8, alt)
    tail_ranks = sum(p <= Fraction(1, 20) for p in p_of_rank)
    result = au.expected_permute(hand, np.ones(len(hand), np.uint32), 16, au.HAND_CASE_MASK, table, len(p_of_rank), tail_ranks, 99, 1)
    identity, rows = au.identity_rows(kind)
    want_main, want_null = au.stage_files(identity, rows, hand, 16, au.HAND_CASE_MASK, alt, Fraction(1, 20), 99, result)
    assert open(out["associate"], "rb").read() == want_main and open(out["null"], "rb").read() == want_null and len(calls) == 1
    assert "Ranking" not in printed and "rank-sum" not in printed and "distinct presence patterns" in printed
    assert "test" not in out["stats"]      # the statistics of the default test are what they were
