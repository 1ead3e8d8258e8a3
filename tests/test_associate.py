"""The permutation null (include/dcrx.h "association") and the `associate` sub-command without a GPU: the exact test against a
brute-force enumeration of labelings, its own identities and scipy; the ranks; the host build of the shared code and of the
primitive's steps (tests/host_assoc) against the contract (tests/assoc_util.py) on every constructed case; the stand-alone
program; the exports; the refusals both entries decide on the host; F = 0 and P = 0 answered on the host; and the stage with
the native call replaced by the contract against files written by hand, its refusals and its help."""
import ctypes as C
import gzip
import itertools
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2


# ---- the exact test ----

@pytest.mark.parametrize("N,n1", [(2, 1), (3, 1), (3, 2), (5, 2), (8, 3), (10, 5), (10, 1), (10, 9)])
def test_fisher_table_is_the_enumeration_of_all_labelings(N, n1):
    """A feature present in the first m samples under every one of the C(N, n1) labelings: the p-value of (m, k) is the share
    of labelings whose table is as extreme as k's."""
    tables = {alt: au.fisher_table(N, n1, alt) for alt in au.ALTERNATIVES}
    for m in range(N + 1):
        ks = [sum(1 for s in L if s < m) for L in itertools.combinations(range(N), n1)]
        count = {k: ks.count(k) for k in set(ks)}
        assert sorted(count) == list(au.feasible(N, n1, m))
        for k in count:
            assert tables["greater"][(m, k)] == Fraction(sum(c for x, c in count.items() if x >= k), len(ks))
            assert tables["less"][(m, k)] == Fraction(sum(c for x, c in count.items() if x <= k), len(ks))
            assert tables["two-sided"][(m, k)] == Fraction(sum(c for c in count.values() if c <= count[k]), len(ks))
    for alt in au.ALTERNATIVES:
        assert asc.fisher_table(N, n1, alt) == tables[alt]      # the stage's table is the contract's


@pytest.mark.parametrize("N,n1", [(64, 32), (64, 20), (16, 8), (8, 3), (33, 1)])
def test_fisher_table_identities(N, n1):
    greater, less, two = (asc.fisher_table(N, n1, alt) for alt in au.ALTERNATIVES)
    assert greater == au.fisher_table(N, n1, "greater") and less == au.fisher_table(N, n1, "less") and two == au.fisher_table(N, n1, "two-sided")
    for m in range(N + 1):
        ks = au.feasible(N, n1, m)
        assert greater[(m, ks[0])] == 1 and less[(m, ks[-1])] == 1
        for k in ks[1:]:
            assert greater[(m, k)] + less[(m, k - 1)] == 1
        for k in ks:
            assert 0 < two[(m, k)] <= 1 and two[(m, k)] >= min(greater[(m, k)], less[(m, k)])
    assert len(greater) == sum(len(au.feasible(N, n1, m)) for m in range(N + 1))


@pytest.mark.parametrize("N,n1", [(64, 32), (64, 20), (16, 8), (8, 3)])
def test_fisher_table_against_scipy(N, n1):
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for alt in au.ALTERNATIVES:
        for (m, k), p in asc.fisher_table(N, n1, alt).items():
            theirs = stats.fisher_exact([[k, n1 - k], [m - k, N - n1 - (m - k)]], alternative=alt)[1]
            worst = max(worst, abs(theirs - float(p)) / float(p))
    print(f"(N, n1) = ({N}, {n1}): the largest relative difference from scipy.stats.fisher_exact is {worst:.3g}")
    assert worst <= 1e-12


def test_ranks_are_dense_and_equal_fractions_share_one():
    for N, n1, alt in ((64, 32, "greater"), (16, 8, "two-sided"), (9, 4, "less"), (2, 1, "greater")):
        table, p_of_rank = asc.rank_table(N, n1, alt)
        cells = au.fisher_table(N, n1, alt)
        want, want_p = au.rank_table(N, n1, alt)
        assert np.array_equal(table.reshape(-1), want) and tuple(p_of_rank) == want_p
        assert list(p_of_rank) == sorted(set(cells.values())) and p_of_rank[-1] == 1
        used = {int(table[m, k]) for (m, k) in cells}
        assert used == set(range(len(p_of_rank)))      # dense
        for (m, k), p in cells.items():
            assert p_of_rank[int(table[m, k])] == p      # equal fractions, one rank; smaller = more extreme
        assert all(int(table[m, k]) == asc.NO_RANK for m in range(N + 1) for k in range(N + 1) if (m, k) not in cells)
    table, p_of_rank = asc.rank_table(64, 32, "greater")
    assert len(p_of_rank) == 514 and sum(p <= Fraction(1, 20) for p in p_of_rank) == 180      # a fact of the arithmetic
    assert len(set(au.fisher_table(16, 8, "two-sided").values())) < len(au.fisher_table(16, 8, "two-sided"))      # shared ranks exist


# ---- the contract's own pieces agree ----

def test_labels_numpy_is_the_sorted_keys():
    for seed, N, n1 in ((0, 2, 1), (1, 33, 16), ((1 << 64) - 1, 64, 63), (7, 64, 1), (9, 31, 30)):
        got = au.labels_numpy(seed, 20, N, n1)
        assert [int(x) for x in got] == [au.labels(seed, p, N, n1) for p in range(20)]
        assert all(bin(int(x)).count("1") == n1 and int(x) >> N == 0 for x in got)
    assert len({int(x) for x in au.labels_numpy(3, 200, 33, 16)}) > 190      # relabelings differ


# ---- the host build: the shared code and the primitive's steps ----

def test_host_selection_score_and_refusals():
    H = au.host_lib()
    for seed, N, n1 in ((0, 2, 1), (5, 33, 17), ((1 << 64) - 1, 64, 63), (7, 64, 1)):
        for p in (0, 1, 255, (1 << 20) - 1):
            assert H.assoc_host_select_labels(seed, p, N, n1) == au.labels(seed, p, N, n1)
    table, _ = au.rank_table(16, 8, "two-sided")
    for M, L in ((0, 0xFF), (0xFFFF, 0xFF), (0x0F0F, 0x00FF), (0x8001, 0x8000)):
        assert H.assoc_host_score(table.ctypes.data, 16, M, L) == int(table[bin(M).count("1") * 17 + bin(M & L).count("1")])
    for N, n1 in ((2, 1), (9, 4), (64, 1), (64, 63)):
        for m in range(N + 1):
            assert [k for k in range(N + 1) if H.assoc_host_feasible(N, n1, m, k)] == list(au.feasible(N, n1, m))
    ok = (16, 0xFF, 10, 81, 5, 100)
    assert H.assoc_host_refuse(*ok) == 0
    for at, value, kind in ((0, 1, 1), (0, 65, 1), (1, 0, 1), (1, 0xFFFF, 1), (1, 1 << 16, 1), (3, 0, 1), (3, 290, 1), (4, 82, 1),
                            (2, 1 << 30, 2), (5, (1 << 20) + 1, 2)):
        args = list(ok)
        args[at] = value
        assert H.assoc_host_refuse(*args) == kind, (at, value)
    assert H.assoc_host_refuse(64, 1 << 63, (1 << 30) - 1, 65 * 65, 65 * 65, 1 << 20) == 0
    assert au.constant("block_perms") == au.constant("lanes") * au.constant("perms_per_lane") and au.constant("lanes") % 64 == 0
    assert au.constant("max_samples") == nat.ASSOC_MAX_SAMPLES and au.constant("max_permutations") == nat.ASSOC_MAX_PERMUTATIONS


@pytest.mark.parametrize("name", au.constructed_names())
def test_host_walk_against_the_contract(name):
    args = au.constructed()[name]
    want = au.expected_permute(*args)
    au.premise(name, args, want)
    got, flushes = au.host_permute(*args)
    au.assert_same(got, want, name)
    F, P, T = len(args[0]), args[7], args[6]
    blocks = -(-F // au.constant("slice")) * -(-P // au.constant("block_perms"))
    assert flushes <= blocks * T      # at most one global add per (block, tail cell)
    assert all(bin(int(x)).count("1") == bin(args[3]).count("1") and int(x) >> args[2] == 0 for x in got["labels"])


def test_the_stand_alone_program_plain():
    """The host walk against the contract written out in C++ in a program of its own (its own main; `make asan` builds the same
    source under AddressSanitizer and UBSan), never loaded into Python."""
    au.host_lib()
    plain = subprocess.run([os.path.join(au.HOST_DIR, "build", "assoc_main")], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "ok", plain.stdout[-2000:]
    assert "one past a slice" in plain.stdout and plain.stdout.count(": 0 differ") == len(plain.stdout.splitlines()) - 1


# ---- exports and ABI ----

def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    for name in ("dcrx_assoc_permute_device", "dcrx_assoc_permute"):
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(nat.lib(), name)
    assert "dcrx_assoc_work_bytes" not in hdr and "THE ENTRY TAKES NO WORK SPACE" in " ".join(hdr.replace("\n *", " ").split())
    assert "#define DCRX_ASSOC_MAX_SAMPLES 64" in hdr and nat.ASSOC_MAX_SAMPLES == 64
    assert "#define DCRX_ASSOC_MAX_PERMUTATIONS (1u << 20)" in hdr and nat.ASSOC_MAX_PERMUTATIONS == 1 << 20
    fields = re.search(r"typedef struct dcrx_assoc_stats \{(.*?)\}", hdr, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == nat.ASSOC_STATS == au.STATS
    assert C.sizeof(nat.AssocStatsC) == 8 * len(nat.ASSOC_STATS)
    assert callable(nat.assoc_permute) and callable(nat.assoc_permute_device)
    makefile = open(os.path.join(ROOT, "decombinator_amd", "csrc", "Makefile")).read()
    assert "dcrx_assoc.hip" in makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"tests", "host_assoc"' in entry


# ---- the refusals of both entries: on the host, before any device call ----

class _Fake:
    """Something with a .ptr: an address the entry must refuse before it looks behind it."""

    def __init__(self, ptr):
        self.ptr = ptr


def _ok_args():
    table, p_of_rank = au.rank_table(16, 8, "greater")
    return {"masks": np.array([0x0F, 0xF0F0], np.uint64), "mults": np.array([1, 2], np.uint32), "n_samples": 16, "case_mask": 0xFF,
            "rank_table": table, "n_ranks": len(p_of_rank), "tail_ranks": 3, "permutations": 5, "seed": 1}


SCALAR_REFUSALS = [
    ({"n_samples": 1, "case_mask": 1}, E_INVALID, "samples"), ({"n_samples": 65}, E_INVALID, "samples"), ({"n_samples": 0}, E_INVALID, "samples"),
    ({"case_mask": 1 << 16}, E_INVALID, "case mask"), ({"case_mask": 0}, E_INVALID, "case"), ({"case_mask": 0xFFFF}, E_INVALID, "case"),
    ({"n_ranks": 0, "tail_ranks": 0}, E_INVALID, "n_ranks"), ({"n_ranks": 17 * 17 + 1}, E_INVALID, "n_ranks"),
    ({"tail_ranks": 10 ** 6}, E_INVALID, "tail_ranks"), ({"permutations": (1 << 20) + 1}, E_UNSUPPORTED, "permutations"),
]


@pytest.mark.parametrize("change,code,word", SCALAR_REFUSALS)
def test_both_entries_refuse_the_scalars(change, code, word):
    a = dict(_ok_args(), **change)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_permute(**a)
    assert e.value.code == code and word in str(e.value) and "dcrx_assoc_permute:" in str(e.value)
    fake = _Fake(0x1000)      # never looked behind: the scalars are judged first
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_permute_device(a["n_samples"], a["case_mask"], 2, fake, fake, fake, a["n_ranks"], a["tail_ranks"], a["permutations"], 1,
                                 fake, fake, fake, fake)
    assert e.value.code == code and word in str(e.value) and "dcrx_assoc_permute_device:" in str(e.value)


def test_both_entries_refuse_too_many_features_and_null_arrays():
    a = _ok_args()
    L, table = nat.lib(), a["rank_table"]
    big = (16, 0xFF, 1 << 30, None, None, table.ctypes.data, a["n_ranks"], 3, 5, 1, None, None, None, None)
    assert L.dcrx_assoc_permute(*big, None) == E_UNSUPPORTED and b"2^30" in L.dcrx_last_error()
    assert L.dcrx_assoc_permute_device(*big, None) == E_UNSUPPORTED and b"2^30" in L.dcrx_last_error()
    ok = [0x1000] * 7      # mask, mult, rank, obs_rank, labels, perm_min, tail
    for missing, F, T, P in ((0, 2, 3, 5), (1, 2, 3, 5), (2, 2, 3, 5), (3, 2, 3, 5), (4, 2, 3, 5), (5, 2, 3, 5), (6, 2, 3, 5), (2, 0, 0, 0)):
        p = list(ok)
        p[missing] = None
        for entry, more in ((L.dcrx_assoc_permute, (None,)), (L.dcrx_assoc_permute_device, (None,))):
            assert entry(16, 0xFF, F, p[0], p[1], p[2], a["n_ranks"], T, P, 1, p[3], p[4], p[5], p[6], *more) == E_INVALID, missing
            assert b"null argument" in L.dcrx_last_error()


def test_the_host_entry_refuses_what_it_sees_in_the_arrays():
    a = _ok_args()
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_permute(**dict(a, masks=np.array([0x0F, 1 << 16], np.uint64)))
    assert e.value.code == E_INVALID and "presence mask" in str(e.value)
    table = a["rank_table"].copy()
    table[8 * 17 + 4] = a["n_ranks"]      # a feasible cell
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_permute(**dict(a, rank_table=table))
    assert e.value.code == E_INVALID and "feasible cell" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_permute(**dict(a, masks=np.array([1, 2, 3], np.uint64), mults=np.array([(1 << 32) - 1, 0, 1], np.uint32)))
    assert e.value.code == E_UNSUPPORTED and "2^32" in str(e.value)
    with pytest.raises(ValueError):
        nat.assoc_permute(**dict(a, mults=np.array([1], np.uint32)))
    with pytest.raises(ValueError):
        nat.assoc_permute(**dict(a, rank_table=table[:-1]))
    with pytest.raises(ValueError):
        nat.assoc_permute(**dict(a, seed=1 << 64))
    for kind, change in (("invalid", {"masks": np.array([0x0F, 1 << 16], np.uint64)}), ("unsupported", {"mults": np.array([(1 << 32) - 1, 1], np.uint32)})):
        with pytest.raises(au.Invalid if kind == "invalid" else au.Unsupported):      # the contract says the same
            b = dict(a, **change)
            au.expected_permute(b["masks"], b["mults"], 16, 0xFF, b["rank_table"], b["n_ranks"], 3, 5, 1)


def test_no_features_or_no_permutations_are_answered_on_the_host():
    """Neither touches a device: both pass where there is none."""
    a = _ok_args()
    empty = dict(a, masks=np.zeros(0, np.uint64), mults=np.zeros(0, np.uint32), permutations=300, seed=(1 << 64) - 1)
    got = nat.assoc_permute(**empty)
    want = au.expected_permute(empty["masks"], empty["mults"], 16, 0xFF, a["rank_table"], a["n_ranks"], 3, 300, (1 << 64) - 1)
    au.assert_same(got, want)
    assert got["stats"] == want["stats"] and (got["perm_min"] == a["n_ranks"]).all() and not got["tail"].any() and len(got["labels"]) == 300
    none = dict(a, permutations=0, masks=au.seeded_masks(16, 500, 4), mults=au.seeded_mults(500, 4))
    got = nat.assoc_permute(**none)
    want = au.expected_permute(none["masks"], none["mults"], 16, 0xFF, a["rank_table"], a["n_ranks"], 3, 0, 1)
    au.assert_same(got, want)
    assert got["stats"] == want["stats"] and got["stats"]["min_perm_rank"] == a["n_ranks"] and len(got["obs_rank"]) == 500
    both = nat.assoc_permute(**dict(empty, permutations=0, tail_ranks=0))
    assert all(len(both[k]) == 0 for k in au.OUTPUTS)


# ---- the stage over the contract ----

def _write(tmp_path, kind="tabulate", gz=False):
    text = au.tabulate_text() if kind == "tabulate" else au.public_text()
    name = ("dcr_tabulate.tsv" if kind == "tabulate" else "dcr_overlap_public.tsv") + (".gz" if gz else "")
    path = tmp_path / name
    path.write_bytes(gzip.compress(text) if gz else text)
    (tmp_path / "cohort.tsv").write_bytes(au.phenotype_text())
    return str(path), str(tmp_path / "cohort.tsv")


def _inp(tmp_path, infile, ph, **more):
    inp = {"command": "associate", "infile": infile, "phenotype": ph, "case": "CMV+", "outpath": str(tmp_path) + os.sep, "prefix": "t_",
           "dontgzip": True, "permutations": 99, "write_null": True}
    inp.update(more)
    return inp


def _run(monkeypatch, inp):
    calls = []
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute(calls))
    return asc.run(inp), calls


def _read(name):
    return gzip.open(name, "rb").read() if name.endswith(".gz") else open(name, "rb").read()


@pytest.mark.parametrize("kind,value,min_count,alternative,gz", [
    ("tabulate", None, 1, None, False), ("public", None, 1, None, False), ("tabulate", "reads", 2, None, False),
    ("public", "reads", 2, "greater", True), ("tabulate", "clonotypes", 1, "less", True), ("tabulate", None, 1, "two-sided", False)])
def test_stage_writes_the_contracts_files(tmp_path, monkeypatch, capsys, kind, value, min_count, alternative, gz):
    infile, ph = _write(tmp_path, kind, gz)
    inp = _inp(tmp_path, infile, ph, value=value, min_count=min_count if min_count != 1 else None, alternative=alternative, dontgzip=not gz)
    out, calls = _run(monkeypatch, inp)
    printed = capsys.readouterr().out
    assert len(calls) == 1      # ONE native call
    masks, mults, N, case_mask, table, n_ranks, tail_ranks, P, seed = calls[0]
    what = value or ("clonotypes" if kind == "tabulate" else "reads")
    hand = au.hand_masks(what, min_count)
    alt = alternative or "greater"
    assert (N, case_mask, P, seed) == (16, au.HAND_CASE_MASK, 99, 1)
    distinct, counts = np.unique(hand, return_counts=True)
    assert np.array_equal(masks, distinct) and np.array_equal(mults, counts)      # de-duplicated by mask
    assert (2 in counts) == (min_count == 1)      # the two features of one mask (under --min-count 2 they part)
    want_table, p_of_rank = au.rank_table(16, 8, alt)
    assert np.array_equal(np.asarray(table).reshape(-1), want_table) and n_ranks == len(p_of_rank)
    assert tail_ranks == sum(p <= Fraction(1, 20) for p in p_of_rank)
    identity, rows = au.identity_rows(kind)
    result = au.expected_permute(hand, np.ones(len(hand), np.uint32), 16, au.HAND_CASE_MASK, want_table, n_ranks, tail_ranks, 99, 1)
    want_main, want_null = au.stage_files(identity, rows, hand, 16, au.HAND_CASE_MASK, alt, Fraction(1, 20), 99, result)
    assert out["associate"].endswith("t_associate.tsv" + (".gz" if gz else "")) and out["null"].endswith("t_associate_null.tsv" + (".gz" if gz else ""))
    assert _read(out["associate"]) == want_main      # byte for byte
    assert _read(out["null"]) == want_null
    lines = want_main.split(b"\n")
    if alt == "greater" and min_count == 1:
        assert lines[1].startswith(rows[0]) and b"\t8\t8\t0\t8\t8\tinf\t7.770008e-05\t" in lines[1]      # exactly the cases: 1 / C(16, 8)
        assert b"\tnan\t1.000000e+00\t" in lines[-2] or b"\tnan\t1.000000e+00\t" in lines[-3]
    assert f"Sample {au.NOT_IN_PH} of" in printed and "left out" in printed
    assert "16 samples used (8 cases, 8 controls; 1 left out without a group, 1 without a row in -ph)" in printed
    assert f"{len(hand)} features ({len(distinct)} distinct presence patterns" in printed and "99 permutations, seed 1" in printed
    assert out["stats"]["features"] == len(hand) and out["stats"]["masks"] == len(distinct)


def test_stage_reads_max_p_exactly_and_takes_the_seed(tmp_path, monkeypatch):
    infile, ph = _write(tmp_path)
    texts = []
    for max_p in ("1/12870", "7.770007770007770e-05", "1", "0"):
        out, calls = _run(monkeypatch, _inp(tmp_path, infile, ph, max_p=max_p, seed=(1 << 64) - 1, ph_sample_column="sample", ph_group_column="group"))
        texts.append((calls[0][6], calls[0][8], _read(out["associate"])))
    assert [t[0] for t in texts] == [1, 0, len(au.rank_table(16, 8, "greater")[1]), 0]      # 1 / C(16, 8) is in; its decimal cut is below it
    assert all(t[1] == (1 << 64) - 1 for t in texts)
    q = [line.split(b"\t")[-1] for line in texts[0][2].split(b"\n")[1:-1]]
    assert q[0] != b"." and set(q[1:]) == {b"."}      # q only where the p-value is at or below --max-p
    assert all(line.split(b"\t")[-1] != b"." for line in texts[2][2].split(b"\n")[1:-1])


def test_stage_without_permutations_makes_no_native_call(tmp_path, monkeypatch):
    infile, ph = _write(tmp_path)

    def boom(*a, **k):
        raise AssertionError("a native entry was called")
    for name in ("assoc_permute", "assoc_permute_device", "lib", "check", "device_count"):
        monkeypatch.setattr(nat, name, boom)
    out = asc.run(_inp(tmp_path, infile, ph, permutations=0))
    identity, rows = au.identity_rows("tabulate")
    want_main, want_null = au.stage_files(identity, rows, au.hand_masks("clonotypes", 1), 16, au.HAND_CASE_MASK, "greater", Fraction(1, 20), 0, None)
    assert open(out["associate"], "rb").read() == want_main and open(out["null"], "rb").read() == want_null
    assert all(line.endswith(b"\t.\t.") for line in want_main.split(b"\n")[1:-1]) and out["result"] is None


def test_stage_through_the_command_line(tmp_path, monkeypatch, capsys):
    infile, ph = _write(tmp_path, gz=True)
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute())
    pipeline.main(["associate", "-in", infile, "-ph", ph, "--case", "CMV-", "-op", str(tmp_path) + os.sep, "--permutations", "50", "--seed", "3"])
    assert "Associated 7 features" in capsys.readouterr().out
    a = _read(str(tmp_path / "dcr_associate.tsv.gz"))
    assert not (tmp_path / "dcr_associate_null.tsv.gz").exists()
    pipeline.main(["associate", "-in", infile, "-ph", ph, "--case", "CMV-", "-op", str(tmp_path) + os.sep, "--permutations", "50", "--seed", "3"])
    assert _read(str(tmp_path / "dcr_associate.tsv.gz")) == a      # a second run gives the same bytes
    assert a.split(b"\n")[1].split(b"\t")[3] == b"CASSMOSTLYCONTROLSF"      # with the controls as cases, that one leads


REFUSALS = [
    ({"infile": None}, "-in"), ({"phenotype": None}, "-ph"), ({"case": None}, "--case"), ({"value": "umis"}, "--value"),
    ({"alternative": "both"}, "--alternative"), ({"min_count": 0}, "--min-count"), ({"permutations": -1}, "--permutations"),
    ({"permutations": (1 << 20) + 1}, "--permutations"), ({"seed": -1}, "--seed"), ({"seed": 1 << 64}, "--seed"),
    ({"max_p": "high"}, "--max-p"), ({"max_p": "1.5"}, "--max-p"), ({"max_p": "-0.1"}, "--max-p"), ({"max_p": "1/0"}, "--max-p"),
]


@pytest.mark.parametrize("change,word", REFUSALS)
def test_stage_refuses_before_a_file_is_opened(tmp_path, monkeypatch, change, word):
    import builtins

    def no_open(*a, **k):
        raise AssertionError("a file was opened")
    inp = dict(_inp(tmp_path, str(tmp_path / "missing.tsv"), str(tmp_path / "missing_too.tsv")), **change)
    assert word in asc.refusal(inp)
    monkeypatch.setattr(builtins, "open", no_open)
    monkeypatch.setattr(gzip, "open", no_open)
    with pytest.raises(ValueError) as e:
        asc.run(inp)
    assert word in str(e.value)


def test_stage_refuses_what_the_files_hold(tmp_path, monkeypatch):
    infile, ph = _write(tmp_path)
    public, _ = _write(tmp_path, "public")
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute())

    def fails(word, **more):
        with pytest.raises(ValueError) as e:
            asc.run(_inp(tmp_path, more.pop("infile", infile), more.pop("phenotype", ph), **more))
        assert word in str(e.value), str(e.value)
    fails("holds reads", infile=public, value="clonotypes")
    other = tmp_path / "other.tsv"
    other.write_bytes(b"clonotype\tv_call\tS00\n0\tTRBV2\t1\n")
    fails("clonotype v_call S00", infile=str(other))      # names the header it found
    fails("'CMV'", case="CMV")
    fails("donor_id", ph_sample_column="donor_id")
    fails("--ph-group-column", ph_group_column="status")

    def cohort(lines):
        path = tmp_path / "c.tsv"
        path.write_text("sample\tgroup\n" + "".join(f"{s}\t{g}\n" for s, g in lines))
        return str(path)
    fails("'S99'", phenotype=cohort([("S00", "CMV+"), ("S01", "CMV-"), ("S99", "CMV-")]))      # no column in -in
    fails("3 labels", phenotype=cohort([("S00", "CMV+"), ("S01", "CMV-"), ("S02", "CMV?")]))
    fails("1 labels", phenotype=cohort([("S00", "CMV+"), ("S01", "CMV+"), ("S02", ".")]))
    fails("two rows", phenotype=cohort([("S00", "CMV+"), ("S01", "CMV-"), ("S00", "CMV-")]))
    bad = tmp_path / "bad.tsv"
    bad.write_bytes(au.tabulate_text().replace(b"\t9\t", b"\tmany\t", 1))
    fails("no count", infile=str(bad), value="reads")
    # two samples are enough; an unknown group may be empty as well as `.`
    out = asc.run(_inp(tmp_path, infile, cohort([("S00", "CMV+"), ("S01", "CMV-"), ("S02", "")]), permutations=5))
    assert out["stats"]["samples"] == 2 and out["stats"]["unknown"] == 1 and out["stats"]["not_in_ph"] == 15


def test_the_help_names_every_flag_and_the_old_parsers_stay(capsys):
    from decombinator_amd.io import cli_args, create_associate_parser, create_parser
    text = " ".join(create_associate_parser().format_help().split())
    for flag in ("-in", "-ph", "--case", "-op", "-pf", "-dz", "--ph-sample-column", "--ph-group-column", "--value", "--min-count",
                 "--alternative", "--permutations", "--seed", "--max-p", "--write-null"):
        assert flag in text, flag
    assert "design choices after Emerson et al., not measured optima" in text and "presence, not abundance" in text
    parser = create_parser()
    subs = [a for a in parser._actions if a.__class__.__name__ == "_SubParsersAction"][0]
    assert list(subs.choices) == ["pipeline", "decombine", "collapse", "translate", "overlap"]
    epilog = parser.epilog
    assert all(word in epilog for word in ("associate", "tabulate", "metaclonotypes", "motifs", "match"))
    old = ("Further commands have parsers of their own: `match` (clonotypes near a database's CDR3s, GPU), `motifs` (CDR3 k-mers enriched "
           "against a background, GPU), `metaclonotypes` (per clonotype the largest CDR3 radius a background still stays out of, GPU) and "
           "`tabulate` (meta-clonotypes counted in bulk samples, GPU); see `python -m decombinator_amd match --help`, `python -m "
           "decombinator_amd motifs --help`, `python -m decombinator_amd metaclonotypes --help` and `python -m decombinator_amd tabulate "
           "--help`.")
    assert epilog.startswith(old)      # every word it had
    inp = cli_args(["associate", "-in", "a.tsv", "-ph", "c.tsv", "--case", "X", "--max-p", "1/20", "--write-null"])
    assert inp["command"] == "associate" and inp["max_p"] == "1/20" and inp["write_null"] and inp["permutations"] is None
    assert asc.DEFAULTS["permutations"] == 10000 and asc.DEFAULTS["alternative"] == "greater" and asc.DEFAULTS["max_p"] == "0.05"
    with pytest.raises(SystemExit):
        pipeline.main(["associate", "-in", "a.tsv", "-ph", "c.tsv"])      # no --case: the parser's error, no file opened
    assert "--case" in capsys.readouterr().err
