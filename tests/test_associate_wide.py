"""The wide permutation null (include/dcrx.h "association, wide") and `associate` on more than 64 samples without a GPU: the
contract in plain Python (tests/assoc_wide_util.py) against the narrow contract; the host build of the shared code and of the
primitive's steps (tests/host_assoc_wide) against it on every constructed case; the stand-alone program; the table builder by
cumulative sums against rank_table and scipy; the exports; the refusals of both entries in their order; F = 0 and P = 0 answered
on the host; and the stage over several tables with the native call replaced by the contract."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import associate as asc
from decombinator_amd import pipeline
from tests import assoc_util as au
from tests import assoc_wide_util as awu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2


# ---- the contract in Python ----

@pytest.mark.parametrize("name", au.constructed_names())
def test_wide_contract_is_the_narrow_contract_up_to_64_samples(name):
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = au.constructed()[name]
    want = au.expected_permute(masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed)
    got = awu.expected_permute_wide(masks.reshape(-1, 1), mults, N, np.array([C_], np.uint64), table.astype(np.uint32), n_ranks, tail_ranks, P, seed)
    assert got["labels"].shape == (P, 1)
    awu.assert_same(got, want, name)
    assert got["stats"] == want["stats"]


def test_words_and_integers():
    x = (0b101 << 128) | (0xFFFF << 60) | 1
    assert awu.to_int(awu.to_words(x, 3)) == x and [int(v) for v in awu.to_words(x, 3)] == [(1 | 0xF << 60), 0xFFF, 0b101]
    assert awu.rows_of([x, 0], 3).shape == (2, 3) and awu.rows_of([], 3).shape == (0, 3)
    got = awu.labels(3, 20, 130, 47)
    assert all(L.bit_count() == 47 and L >> 130 == 0 for L in got) and len(set(got)) == 20


# ---- the host build: the shared code and the primitive's steps ----

def test_host_selection_sizes_and_refusals():
    H = awu.host_lib()
    for seed, N, n1 in ((0, 2, 1), (5, 65, 17), ((1 << 64) - 1, 128, 127), (7, 129, 1), (11, 1000, 400), (13, 1024, 512)):
        words = np.zeros(awu.words_for(N), np.uint64)
        for p in (0, 1, (1 << 20) - 1):
            H.assoc_wide_host_select_labels(seed, p, N, n1, words.ctypes.data)
            assert awu.to_int(words) == awu.label(seed, p, N, n1)
    for N in (2, 63, 64, 65, 128, 129, 1023, 1024):
        W = awu.words_for(N)
        assert awu.constant("words_for", N) == W
        assert sum(int(H.assoc_wide_host_word_bits(N, w)) << (64 * w) for w in range(W)) == (1 << N) - 1
        assert int(H.assoc_wide_host_word_bits(N, W)) == 0
    assert [awu.constant("perms_per_lane", W) for W in range(1, 17)] == [4] * 4 + [2] * 4 + [1] * 8
    assert all(awu.constant("block_perms", W) == awu.constant("lanes") * awu.constant("perms_per_lane", W) for W in range(1, 17))
    assert awu.constant("lanes") % 64 == 0 and awu.constant("max_samples") == nat.ASSOC_WIDE_MAX_SAMPLES == 1024
    assert awu.constant("max_permutations") == nat.ASSOC_MAX_PERMUTATIONS
    ok = (200, 10, 81, 5, 100)      # N, F, n_ranks, tail_ranks, P
    assert H.assoc_wide_host_refuse(*ok) == 0
    for at, value, kind in ((0, 1, 1), (0, 1025, 1), (2, 0, 1), (2, 201 * 201 + 1, 1), (3, 82, 1), (1, 1 << 30, 2), (4, (1 << 20) + 1, 2)):
        args = list(ok)
        args[at] = value
        assert H.assoc_wide_host_refuse(*args) == kind, (at, value)
    assert H.assoc_wide_host_refuse(1024, (1 << 30) - 1, 1025 * 1025, 1025 * 1025, 1 << 20) == 0
    assert H.assoc_wide_host_refuse(1, 1 << 30, 0, 1, (1 << 20) + 1) == 1      # the samples first ...
    assert H.assoc_wide_host_refuse(200, 1 << 30, 0, 1, (1 << 20) + 1) == 1     # ... then the ranks, then the sizes
    assert H.assoc_wide_host_refuse(200, 1 << 30, 5, 1, (1 << 20) + 1) == 2

    def cases(N, x, strict):
        return H.assoc_wide_host_refuse_cases(N, awu.to_words(x, awu.words_for(N)).ctypes.data, strict)
    assert cases(130, 0b11 << 128, 1) == 0 and cases(130, 1 << 130, 1) == 1 and cases(130, (1 << 130) | 1, 0) == 0
    assert cases(130, 0, 1) == 1 and cases(130, (1 << 130) - 1, 0) == 1 and cases(130, 1 << 130, 0) == 1      # cut to N bits: no case


@pytest.mark.parametrize("name", awu.constructed_names())
def test_host_walk_against_the_contract(name):
    args = awu.constructed()[name]
    want = awu.expected_permute_wide(*args)
    awu.premise(name, args, want)
    got, flushes, runs = awu.host_permute(*args)
    awu.assert_same(got, want, name)
    masks, N, P = args[0], args[2], args[7]
    F, W = len(masks), awu.words_for(N)
    weighted = [awu.to_int(r).bit_count() for r, w in zip(masks, args[1]) if w]
    blocks_y = -(-P // awu.constant("block_perms", W))
    changes = 0
    for a in range(0, len(args[1]), awu.constant("slice")):      # the runs of equal popcount of every slice's weighted features
        ms = [awu.to_int(r).bit_count() for r, w in zip(masks[a:a + awu.constant("slice")], args[1][a:a + awu.constant("slice")]) if w]
        changes += sum(1 for i, m in enumerate(ms) if i == 0 or m != ms[i - 1])
    assert runs == (changes * blocks_y if P else 0)
    assert flushes <= runs * (max(weighted, default=0) + 1)      # at most one global add per (run, cell of its row)
    n1 = awu.to_int(args[3]).bit_count()
    assert all(awu.to_int(r).bit_count() == n1 and awu.to_int(r) >> N == 0 for r in got["labels"])
    if name == "ascending_popcount":
        other = awu.host_permute(*awu.constructed()["shuffled_popcount"])
        assert runs < other[2] // 10      # sorted input: a handful of runs a slice; shuffled: nearly one a feature
        for key in ("perm_min", "tail", "labels"):      # the same features in another order: the same null
            assert np.array_equal(got[key], other[0][key])


def test_the_stand_alone_program_plain():
    """The host walk against the contract written out in C++ in a program of its own (its own main; `make asan` builds the same
    source under AddressSanitizer and UBSan), never loaded into Python."""
    awu.host_lib()
    plain = subprocess.run([awu.HOST_MAIN], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "ok", plain.stdout[-2000:]
    assert "sixteen words" in plain.stdout and plain.stdout.count(": 0 differ") == len(plain.stdout.splitlines()) - 1
    makefile = open(os.path.join(awu.HOST_DIR, "Makefile")).read()
    assert "asan:" in makefile and "-fsanitize=address,undefined" in makefile and "LD_PRELOAD" not in makefile


# ---- the table builder ----

@pytest.mark.parametrize("N,n1", [(64, 32), (64, 20), (16, 8), (8, 3), (2, 1)])
def test_table_by_cumulative_sums_is_rank_table(N, n1):
    for alt in au.ALTERNATIVES:
        want, want_p = asc.rank_table(N, n1, alt)
        table, p_of_rank = asc.rank_table_sums(N, n1, alt)
        assert table.dtype == np.uint32 and table.shape == (N + 1, N + 1)
        assert list(p_of_rank) == list(want_p) and all(type(p) is Fraction for p in p_of_rank)      # the very same Fractions
        cells = {(m, k) for m in range(N + 1) for k in au.feasible(N, n1, m)}
        for m in range(N + 1):
            for k in range(N + 1):
                if (m, k) in cells:
                    assert int(table[m, k]) == int(want[m, k])      # the very same dense ranks
                else:
                    assert int(table[m, k]) == asc.NO_RANK_WIDE and int(want[m, k]) == asc.NO_RANK


@pytest.mark.parametrize("N,n1", [(130, 47), (200, 77)])
def test_table_by_cumulative_sums_against_scipy(N, n1):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(N)
    worst = 0.0
    for alt in au.ALTERNATIVES:
        table, p_of_rank = asc.rank_table_sums(N, n1, alt)
        cells = [(m, k) for m in (0, 1, n1, N - n1, N // 2, N - 1, N) for k in (au.feasible(N, n1, m)[0], au.feasible(N, n1, m)[-1])]
        cells += [(int(m), int(rng.integers(au.feasible(N, n1, int(m))[0], au.feasible(N, n1, int(m))[-1] + 1))) for m in rng.integers(2, N - 1, 12)]
        for m, k in cells:
            p = p_of_rank[int(table[m, k])]
            theirs = stats.fisher_exact([[k, n1 - k], [m - k, N - n1 - (m - k)]], alternative=alt)[1]
            worst = max(worst, abs(theirs - float(p)) / float(p))
    print(f"(N, n1) = ({N}, {n1}): the largest relative difference from scipy.stats.fisher_exact is {worst:.3g}")
    assert worst <= 1e-12


def test_two_sided_rows_share_a_rank_where_h_is_equal():
    from math import comb
    for N, n1 in ((130, 65), (70, 27), (66, 3)):
        table, p_of_rank = asc.rank_table_sums(N, n1, "two-sided")
        shared = 0
        for m in (1, 2, N // 2, N // 2 + 1, N - 3):
            ks = au.feasible(N, n1, m)
            h = {k: comb(n1, k) * comb(N - n1, m - k) for k in ks}
            for a in ks:
                for b in ks:
                    assert (h[a] == h[b]) <= (table[m, a] == table[m, b])      # equal h: one rank
                    assert (h[a] < h[b]) <= (table[m, a] < table[m, b])        # the likelier table, the larger p
                    shared += a != b and h[a] == h[b]
                assert p_of_rank[int(table[m, a])] == Fraction(sum(x for x in h.values() if x <= h[a]), comb(N, m))
        assert shared or n1 * 2 != N      # a balanced cohort's rows are symmetric: k and m - k share a rank
    table, p_of_rank = asc.rank_table_sums(200, 100, "greater")
    assert len(p_of_rank) == 5002 and sum(p <= Fraction(1, 20) for p in p_of_rank) == 2066      # facts of the arithmetic


# ---- exports and ABI ----

def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "#define DCRX_ABI_VERSION 5" in hdr and nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    for name in ("dcrx_assoc_permute_wide_device", "dcrx_assoc_permute_wide"):
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(nat.lib(), name)
    assert "#define DCRX_ASSOC_WIDE_MAX_SAMPLES 1024" in hdr and nat.ASSOC_WIDE_MAX_SAMPLES == 1024
    assert "#define DCRX_ASSOC_MAX_SAMPLES 64" in hdr and nat.ASSOC_MAX_SAMPLES == 64      # the narrow layer stays
    assert "---- association, wide" in hdr and "dcrx_assoc_wide_work_bytes" not in hdr
    assert flat.count("THE ENTRY TAKES NO WORK SPACE") >= 2      # the narrow primitive's and the wide one's
    wide = flat[flat.index("---- association, wide"):flat.index("---- the CDR3 network, weighted")]
    for words in ("bit s & 63 of word s >> 6", "UINT32", "IN HOST MEMORY", "in this order", "ORDER OF THE FEATURES", "k <= m <= N"):
        assert words in wide, words
    assert callable(nat.assoc_permute_wide) and callable(nat.assoc_permute_wide_device)
    makefile = open(os.path.join(ROOT, "decombinator_amd", "csrc", "Makefile")).read()
    assert "dcrx_assoc_wide.hip" in makefile and "dcrx_assoc.hip" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"tests", "host_assoc_wide"' in entry and '"tests", "host_assoc"' in entry
    core = open(os.path.join(ROOT, "decombinator_amd", "csrc", "dcrx_assoc_wide_core.h")).read()
    assert "cannot wrap" in core and "static_assert((uint64_t)SLICE * MAX_BLOCK_PERMS * (MAX_WEIGHT - 1) < (1ull << 63)" in core


# ---- the refusals of both entries: on the host, before any device call, in the header's order ----

def _ok():
    table, n_ranks = awu.census_table(130, 60)
    return {"masks": awu.rows_of([0x0F, 0xF0F0 << 100], 3), "mults": np.array([1, 2], np.uint32), "n_samples": 130,
            "case_words": awu.to_words(au.half_cases(130, 60), 3), "rank_table": table, "n_ranks": n_ranks, "tail_ranks": 3, "permutations": 5,
            "seed": 1}


def _both(a, cases=None, pointers=None):
    """(code, message) of the host entry and of the device entry on the same scalars, with addresses that must not be looked
    behind before the refusal (pointers: mask, mult, rank, obs_rank, labels, perm_min, tail)."""
    L = nat.lib()
    cw = np.ascontiguousarray(a["case_words"], np.uint64) if cases is None else cases
    p = [0x1000] * 7 if pointers is None else pointers
    out = []
    for entry, last in ((L.dcrx_assoc_permute_wide, None), (L.dcrx_assoc_permute_wide_device, None)):
        rc = entry(a["n_samples"], cw.ctypes.data, a.get("F", 2), p[0], p[1], p[2], a["n_ranks"], a["tail_ranks"],
                   a["permutations"], a["seed"], p[3], p[4], p[5], p[6], last)
        out.append((rc, L.dcrx_last_error().decode()))
    return out


SCALAR_REFUSALS = [
    ({"n_samples": 1}, E_INVALID, "samples"), ({"n_samples": 1025}, E_INVALID, "samples"), ({"n_samples": 0}, E_INVALID, "samples"),
    ({"n_ranks": 0, "tail_ranks": 0}, E_INVALID, "n_ranks"), ({"n_ranks": 131 * 131 + 1}, E_INVALID, "n_ranks"),
    ({"tail_ranks": 10 ** 6}, E_INVALID, "tail_ranks"), ({"F": 1 << 30}, E_UNSUPPORTED, "2^30"),
    ({"permutations": (1 << 20) + 1}, E_UNSUPPORTED, "permutations"),
    # the order: samples, n_ranks, tail_ranks, features, permutations
    ({"n_samples": 1025, "n_ranks": 0, "F": 1 << 30}, E_INVALID, "samples"), ({"n_ranks": 0, "tail_ranks": 7, "F": 1 << 30}, E_INVALID, "n_ranks"),
    ({"tail_ranks": 10 ** 6, "F": 1 << 30}, E_INVALID, "tail_ranks"), ({"F": 1 << 30, "permutations": (1 << 20) + 1}, E_UNSUPPORTED, "2^30"),
]


@pytest.mark.parametrize("change,code,word", SCALAR_REFUSALS)
def test_both_entries_refuse_the_scalars_first(change, code, word):
    for entry, (rc, msg) in zip(("dcrx_assoc_permute_wide:", "dcrx_assoc_permute_wide_device:"), _both(dict(_ok(), **change), pointers=[None] * 7)):
        assert rc == code and word in msg and entry in msg, (rc, msg)      # (null arrays too: the scalars come first)


def test_both_entries_refuse_null_arrays_then_the_case_mask():
    a = _ok()
    for missing, F, T, P in ((0, 2, 3, 5), (1, 2, 3, 5), (2, 2, 3, 5), (3, 2, 3, 5), (4, 2, 3, 5), (5, 2, 3, 5), (6, 2, 3, 5), (2, 0, 0, 0)):
        p = [0x1000] * 7
        p[missing] = None
        none = awu.to_words(0, 3)      # a case mask without a case: judged after the null arrays
        for rc, msg in _both(dict(a, F=F, tail_ranks=T, permutations=P), cases=none, pointers=p):
            assert rc == E_INVALID and "null argument" in msg, (missing, msg)
    L = nat.lib()
    for entry in (L.dcrx_assoc_permute_wide, L.dcrx_assoc_permute_wide_device):      # the case mask is an array of its own
        assert entry(130, None, 2, 0x1000, 0x1000, 0x1000, a["n_ranks"], 3, 5, 1, 0x1000, 0x1000, 0x1000, 0x1000, None) == E_INVALID
        assert b"null argument" in L.dcrx_last_error()
    # the case mask, with nothing null: no case and no control in both entries
    for x in (0, (1 << 130) - 1):
        for rc, msg in _both(a, cases=awu.to_words(x, 3)):
            assert rc == E_INVALID and "1 .. N - 1 cases" in msg, msg
    # a bit at or above N: the host entry refuses it; the device entry cuts it off, so a mask of that bit alone holds no case
    host, device = _both(a, cases=awu.to_words(1 << 130, 3))
    assert host[0] == E_INVALID and "case mask has a bit at or above" in host[1]
    assert device[0] == E_INVALID and "1 .. N - 1 cases" in device[1]


def test_the_host_entry_refuses_what_it_sees_in_the_arrays_in_order():
    a = _ok()
    bad_mask = awu.rows_of([0x0F, 1 << 130], 3)
    bad_table = a["rank_table"].copy()
    n1 = awu.to_int(a["case_words"]).bit_count()
    bad_table[64 * 131 + au.feasible(130, n1, 64)[3]] = a["n_ranks"]      # a feasible cell
    heavy = np.array([(1 << 32) - 1, 1], np.uint32)
    with pytest.raises(nat.DcrxError) as e:      # the case-mask bit before everything the arrays hold
        nat.assoc_permute_wide(**dict(a, case_words=awu.to_words((1 << 130) | 1, 3), rank_table=bad_table, masks=bad_mask, mults=heavy))
    assert e.value.code == E_INVALID and "case mask has a bit" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:      # then the table
        nat.assoc_permute_wide(**dict(a, rank_table=bad_table, masks=bad_mask, mults=heavy))
    assert e.value.code == E_INVALID and "feasible cell" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:      # then the masks
        nat.assoc_permute_wide(**dict(a, masks=bad_mask))
    assert e.value.code == E_INVALID and "presence mask" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:      # ... every mask, also where the sum passes 2^32 at an earlier feature
        nat.assoc_permute_wide(**dict(a, masks=awu.rows_of([1, 2, 1 << 130], 3), mults=np.array([(1 << 32) - 1, 1, 0], np.uint32)))
    assert e.value.code == E_INVALID and "presence mask" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:      # then the multiplicities
        nat.assoc_permute_wide(**dict(a, mults=heavy))
    assert e.value.code == E_UNSUPPORTED and "2^32" in str(e.value)
    unused = a["rank_table"].copy()
    unused[a["rank_table"] == awu.NO_RANK] = 0xFFFFFFFF      # cells no cohort produces may hold anything: P = 0 runs on the host
    assert len(nat.assoc_permute_wide(**dict(a, rank_table=unused, permutations=0))["obs_rank"]) == 2
    for change in ({"mults": np.array([1], np.uint32)}, {"rank_table": bad_table[:-1]}, {"seed": 1 << 64}, {"masks": awu.rows_of([1, 2], 2)},
                   {"case_words": awu.to_words(1, 2)}, {"case_words": 1 << 192}):
        with pytest.raises(ValueError):
            nat.assoc_permute_wide(**dict(a, **change))
    for kind, change in ((au.Invalid, {"masks": bad_mask}), (au.Unsupported, {"mults": heavy}), (au.Invalid, {"rank_table": bad_table}),
                         (au.Invalid, {"case_words": awu.to_words(1 << 130, 3)})):
        with pytest.raises(kind):      # the contract says the same
            b = dict(a, **change)
            awu.expected_permute_wide(b["masks"], b["mults"], 130, b["case_words"], b["rank_table"], b["n_ranks"], 3, 5, 1)


def test_no_features_or_no_permutations_are_answered_on_the_host():
    """Neither touches a device: both pass where there is none."""
    a = _ok()
    empty = dict(a, masks=np.zeros((0, 3), np.uint64), mults=np.zeros(0, np.uint32), permutations=300, seed=(1 << 64) - 1)
    got = nat.assoc_permute_wide(**empty)
    want = awu.expected_permute_wide(empty["masks"], empty["mults"], 130, a["case_words"], a["rank_table"], a["n_ranks"], 3, 300, (1 << 64) - 1)
    awu.assert_same(got, want)
    assert got["stats"] == want["stats"] and (got["perm_min"] == a["n_ranks"]).all() and not got["tail"].any() and got["labels"].shape == (300, 3)
    none = dict(a, permutations=0, masks=awu.seeded_rows(130, 500, 4), mults=au.seeded_mults(500, 4))
    got = nat.assoc_permute_wide(**none)
    want = awu.expected_permute_wide(none["masks"], none["mults"], 130, a["case_words"], a["rank_table"], a["n_ranks"], 3, 0, 1)
    awu.assert_same(got, want)
    assert got["stats"] == want["stats"] and got["stats"]["min_perm_rank"] == a["n_ranks"] and len(got["obs_rank"]) == 500
    both = nat.assoc_permute_wide(**dict(empty, permutations=0, tail_ranks=0))
    assert all(len(both[k]) == 0 for k in au.OUTPUTS)
    table, n_ranks = awu.census_table(1024, 512)      # sixteen words, one Python integer as the case mask
    got = nat.assoc_permute_wide(np.zeros((0, 16), np.uint64), np.zeros(0, np.uint32), 1024, au.half_cases(1024, 512), table, n_ranks, n_ranks, 3, 9)
    assert [awu.to_int(r) for r in got["labels"]] == list(awu.labels(9, 3, 1024, 512)) and len(got["tail"]) == 263169


# ---- the stage over the contract ----

def _write(tmp_path, parts):
    """The hand-written cohort as tabulate.tsv files, one per list of samples: (the files' names, the phenotype's)."""
    names = []
    for n, samples in enumerate(parts):
        path = tmp_path / f"run{n}_tabulate.tsv"
        path.write_bytes(awu.tabulate_text(samples))
        names.append(str(path))
    (tmp_path / "cohort.tsv").write_bytes(awu.phenotype_text())
    return names, str(tmp_path / "cohort.tsv")


def _inp(tmp_path, infile, ph, **more):
    inp = {"command": "associate", "infile": infile, "phenotype": ph, "case": "CMV+", "outpath": str(tmp_path) + os.sep, "prefix": "t_",
           "dontgzip": True, "permutations": 99, "write_null": True}
    inp.update(more)
    return inp


def _boom(*a, **k):
    raise AssertionError("a native entry was called")


def _want_files(alt, P, result):
    identity, rows = awu.identity_rows()
    return au.stage_files(identity, rows, awu.hand_masks(), 70, awu.HAND_CASE_MASK, alt, Fraction(1, 20), P, result)


@pytest.mark.parametrize("alternative", au.ALTERNATIVES)
def test_stage_joins_two_tables_and_writes_the_contracts_files(tmp_path, monkeypatch, capsys, alternative):
    files, ph = _write(tmp_path, [awu.FIRST, awu.SECOND])
    calls = []
    monkeypatch.setattr(nat, "assoc_permute_wide", awu.python_permute_wide(calls))
    monkeypatch.setattr(nat, "assoc_permute", _boom)
    out = asc.run(_inp(tmp_path, files, ph, alternative=alternative))
    printed = capsys.readouterr().out
    assert len(calls) == 1      # ONE native call, the wide one
    masks, mults, N, case_words, table, n_ranks, tail_ranks, P, seed = calls[0]
    hand = awu.hand_masks()
    assert (N, awu.to_int(case_words), P, seed) == (70, awu.HAND_CASE_MASK, 99, 1) and masks.shape[1] == 2
    got = [awu.to_int(r) for r in masks]
    assert sorted(got) == sorted(set(hand)) and len(got) == len(hand) - 1      # de-duplicated by row: one_mask_a and _b are one
    assert [x.bit_count() for x in got] == sorted(x.bit_count() for x in got)      # handed over in ascending popcount
    assert sorted(int(x) for x in mults) == [1] * (len(got) - 1) + [2]
    want_table, want_ranks, want_tail = awu.exact_table(70, 27, alternative)
    assert np.array_equal(np.asarray(table).reshape(-1), want_table) and (n_ranks, tail_ranks) == (want_ranks, want_tail)
    result = awu.expected_permute_wide(awu.rows_of(hand, 2), np.ones(len(hand), np.uint32), 70, awu.HAND_CASE_MASK, want_table, n_ranks, tail_ranks, 99, 1)
    want_main, want_null = _want_files(alternative, 99, result)
    assert open(out["associate"], "rb").read() == want_main      # byte for byte
    assert open(out["null"], "rb").read() == want_null
    assert f"Sample {awu.NOT_IN_PH} of {files[0]}, {files[1]} has no row in" in printed and "left out" in printed
    assert "70 samples used (27 cases, 43 controls; 1 left out without a group, 1 without a row in -ph)" in printed
    assert f"{len(hand)} features ({len(got)} distinct presence patterns" in printed and "Building the table" not in printed
    # the same cohort given as ONE table of 72 columns: the same bytes
    one = [str(tmp_path / "all_tabulate.tsv")]
    (tmp_path / "all_tabulate.tsv").write_bytes(awu.tabulate_text(awu.FIRST + awu.SECOND))
    for infile in (one[0], one):      # a string or a list
        again = asc.run(_inp(tmp_path, infile, ph, alternative=alternative, prefix="one_"))
        assert open(again["associate"], "rb").read() == want_main and open(again["null"], "rb").read() == want_null
    assert len(calls) == 3 and all(np.array_equal(c[0], calls[0][0]) for c in calls[1:])


def test_stage_through_the_command_line_takes_several_tables(tmp_path, monkeypatch, capsys):
    files, ph = _write(tmp_path, [awu.FIRST, awu.SECOND])
    monkeypatch.setattr(nat, "assoc_permute_wide", awu.python_permute_wide())
    pipeline.main(["associate", "-in", files[0], files[1], "-ph", ph, "--case", "CMV+", "-op", str(tmp_path) + os.sep, "-dz", "--permutations", "50"])
    assert "Associated 11 features" in capsys.readouterr().out
    text = open(tmp_path / "dcr_associate.tsv", "rb").read()
    assert text.split(b"\n")[1].split(b"\t")[3] == b"CASSEXACTLYTHECASESF"
    from decombinator_amd.io import create_associate_parser
    assert "Several tabulate.tsv" in " ".join(create_associate_parser().format_help().split())


@pytest.mark.parametrize("n_samples,files", [(70, 2), (200, 4)])
def test_stage_without_permutations_needs_no_native_entry(tmp_path, monkeypatch, n_samples, files):
    for name in ("assoc_permute", "assoc_permute_device", "assoc_permute_wide", "assoc_permute_wide_device", "lib", "check", "device_count"):
        monkeypatch.setattr(nat, name, _boom)
    if n_samples == 70:
        names, ph = _write(tmp_path, [awu.FIRST, awu.SECOND])
        out = asc.run(_inp(tmp_path, names, ph, permutations=0))
        want_main, want_null = _want_files("greater", 0, None)
        assert open(out["associate"], "rb").read() == want_main and open(out["null"], "rb").read() == want_null
    else:
        tables, ph_text, samples, where = awu.wide_cohort_texts(n_samples, files)
        names = []
        for n, text in enumerate(tables):
            (tmp_path / f"r{n}.tsv").write_bytes(text)
            names.append(str(tmp_path / f"r{n}.tsv"))
        (tmp_path / "ph.tsv").write_bytes(ph_text)
        out = asc.run(_inp(tmp_path, names, str(tmp_path / "ph.tsv"), permutations=0))
        lines = open(out["associate"], "rb").read().split(b"\n")[1:-1]
        assert out["stats"]["samples"] == 200 and out["stats"]["cases"] == 67 and len(lines) == 3
        first = lines[0].split(b"\t")      # exactly the cases leads: 1 / C(200, 67)
        from math import comb
        assert first[3] == b"CASSQF" and first[5:10] == [b"67", b"67", b"0", b"67", b"133"] and first[10] == b"inf"
        assert first[11] == format(1 / comb(200, 67), ".6e").encode()
    assert all(line.endswith(b"\t.\t.") for line in open(out["associate"], "rb").read().split(b"\n")[1:-1]) and out["result"] is None


def test_the_joins_refusals(tmp_path, monkeypatch):
    files, ph = _write(tmp_path, [awu.FIRST, awu.SECOND])
    monkeypatch.setattr(nat, "assoc_permute_wide", _boom)
    monkeypatch.setattr(nat, "assoc_permute", _boom)

    def fails(infile, *words):
        with pytest.raises(ValueError) as e:
            asc.run(_inp(tmp_path, infile, ph))
        assert all(w in str(e.value) for w in words), str(e.value)
    other = tmp_path / "other_tabulate.tsv"
    lines = awu.tabulate_text(awu.SECOND).split(b"\n")
    lines[4] = lines[4].replace(b"CASSTHELASTSIXF", b"CASSTHELASTSEVENF")
    other.write_bytes(b"\n".join(lines))
    fails([files[0], str(other)], str(other) + ", line 5", files[0])      # the first file and line that differ
    other.write_bytes(b"\n".join(lines[:3] + lines[4:]))                  # a line short: line 4 differs first
    fails([files[0], str(other)], str(other) + ", line 4")
    other.write_bytes(b"\n".join(awu.tabulate_text(awu.SECOND).split(b"\n")[:-3]) + b"\n")      # fewer meta-clonotypes
    fails([files[0], str(other)], str(other) + ", line 11", "9 meta-clonotypes")
    other.write_bytes(awu.tabulate_text(awu.SECOND[:5] + ["A03"]))
    fails([files[0], str(other)], "'A03'", files[0], str(other))          # a sample in two files
    fails([files[0], files[0]], "'A00'")
    public = tmp_path / "dcr_overlap_public.tsv"
    public.write_bytes(au.public_text())
    for infile in ([str(public), str(public)], [files[0], str(public)]):
        fails(infile, "overlap_public.tsv", "--min-samples")               # refused, with the reason
    fails([], "-in")


def test_1025_samples_are_refused_and_64_used_call_the_narrow_entry(tmp_path, monkeypatch):
    tables, ph_text, samples, where = awu.wide_cohort_texts(1025, 17)
    names = []
    for n, text in enumerate(tables):
        (tmp_path / f"r{n}.tsv").write_bytes(text)
        names.append(str(tmp_path / f"r{n}.tsv"))
    (tmp_path / "ph.tsv").write_bytes(ph_text)
    monkeypatch.setattr(nat, "assoc_permute_wide", _boom)
    with pytest.raises(ValueError) as e:
        asc.run(_inp(tmp_path, names, str(tmp_path / "ph.tsv"), permutations=0))
    assert "1025" in str(e.value) and "1024" in str(e.value)
    # exactly 64 used samples out of two files (40 + 30 columns, six more without a group): the NARROW entry, the wide one raises
    files, _ = _write(tmp_path, [awu.FIRST, awu.SECOND])
    drop = set(awu.USED[34:40])
    ph = awu.phenotype_text().decode().split("\n")
    (tmp_path / "c64.tsv").write_text("\n".join("\t".join(f[:3] + ["."]) if f[1] in drop else "\t".join(f) for f in (x.split("\t") for x in ph[:-1])) + "\n")
    calls = []
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute(calls))
    out = asc.run(_inp(tmp_path, files, str(tmp_path / "c64.tsv")))
    assert len(calls) == 1 and calls[0][2] == 64 and np.asarray(calls[0][0]).ndim == 1 and np.asarray(calls[0][4]).dtype == np.uint16
    used = [s for s in awu.USED if s not in drop]
    cases = sum(1 << i for i, s in enumerate(used) if s in awu.CASES)
    assert calls[0][3] == cases and isinstance(calls[0][3], int)
    hand = [sum(1 << i for i, s in enumerate(used) if where_.get(s, (0, 0))[0] >= 1) for _, where_ in awu.FEATURES]
    identity, rows = awu.identity_rows()
    table, p_of_rank = au.rank_table(64, bin(cases).count("1"), "greater")
    result = au.expected_permute(np.array(hand, np.uint64), np.ones(len(hand), np.uint32), 64, cases, table, len(p_of_rank),
                                 sum(p <= Fraction(1, 20) for p in p_of_rank), 99, 1)
    want_main, want_null = au.stage_files(identity, rows, hand, 64, cases, "greater", Fraction(1, 20), 99, result)
    assert open(out["associate"], "rb").read() == want_main and open(out["null"], "rb").read() == want_null
