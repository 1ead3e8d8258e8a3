"""`motifs --groups` without a GPU: the contract in Python (gu.expected_groups) on hand-made tables whose answers are written out
here; the selection rule on hand values; the stage with the native calls replaced by the contract — both files byte for byte,
the order of their lines, `.` for no motif, gzip, the printed line, every new refusal, and a run without --groups that writes
what it wrote before —; the help texts; the exports; the stand-alone host program of the shared header's new code."""
import gzip
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import motifs, pipeline
from tests import motif_groups_util as gu
from tests import motif_util as mu
from tests import test_motifs as cpu
from tests.test_motifs import stage      # noqa: F401  (the fixture: samples A and B and the background as files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sel(*letters):
    """(k, code) of motifs given as letters, in motif order."""
    return sorted(((len(w), mu.code_of(w.encode())) for w in letters), key=lambda kc: gu.motif_number(*kc))


def ints(a):
    return [int(x) for x in a]


# ---- the contract on hand-made tables ----

def test_contract_a_motif_twice_in_one_unit_is_one_member():
    units = [b"XXXABABXXX", b"XXXQQQQXXX", b"XXXCABCXXX"]
    got = gu.expected_groups(units, [5, 7, 11], ks=(2,), trim=(3, 3), selected=sel("AB"), G=0)
    assert ints(got["mem_off"]) == [0, 2] and ints(got["mem"]) == [0, 2] and got["need"] == 2
    assert ints(got["n_motifs"]) == [1, 0, 1] and ints(got["group_of"]) == [0, 1, 0]
    assert (ints(got["head"]), ints(got["units"]), ints(got["weight"])) == ([0, 1], [2, 1], [16, 7])
    assert got["stats"]["mixed_groups"] == 0 and got["stats"]["singleton_groups"] == 1 and got["stats"]["largest_group"] == 2


def test_contract_a_unit_too_short_for_a_window_takes_part_and_holds_nothing():
    units = [b"CASABF", b"XXXABXXX", b"XXXABYYY"]      # six letters under 3,3: no window, though it reads AB
    got = gu.expected_groups(units, [1, 1, 1], ks=(2,), trim=(3, 3), selected=sel("AB"), G=1)
    assert ints(got["mem"]) == [1, 2] and ints(got["n_motifs"]) == [0, 1, 1] and ints(got["group_of"]) == [0, 1, 1]
    assert got["stats"]["take_part"] == 3 and ints(got["degree"]) == [0, 0, 0]


def test_contract_a_chain_over_both_kinds_of_edge_is_one_group():
    """unit 0 -AB- unit 1 =one residue= unit 2 -CD- unit 3; unit 4 stands alone.  ABD to ACD takes AB away and brings CD."""
    units = [b"XXXABXXX", b"QQQABDQQQ", b"QQQACDQQQ", b"TTTCDTTT", b"PPPPPPPP"]
    weights = [1, 2, 4, 8, 16]
    got = gu.expected_groups(units, weights, ks=(2,), trim=(3, 3), selected=sel("AB", "CD"), G=1)
    assert ints(got["mem_off"]) == [0, 2, 4] and ints(got["mem"]) == [0, 1, 2, 3] and ints(got["n_motifs"]) == [1, 1, 1, 1, 0]
    assert ints(got["degree"]) == [0, 1, 1, 0, 0] and got["stats"]["global_edges"] == 1
    assert ints(got["group_of"]) == [0, 0, 0, 0, 1] and ints(got["head"]) == [0, 4] and ints(got["units"]) == [4, 1]
    assert ints(got["weight"]) == [15, 16] and got["stats"]["mixed_groups"] == 1 and got["stats"]["largest_group"] == 4
    apart = gu.expected_groups(units, weights, ks=(2,), trim=(3, 3), selected=sel("AB", "CD"), G=0)      # without the middle link: two groups
    assert ints(apart["group_of"]) == [0, 0, 1, 1, 2] and ints(apart["weight"]) == [3, 12, 16] and apart["stats"]["mixed_groups"] == 0
    only = gu.expected_groups(units, weights, ks=(2,), trim=(3, 3), selected=[], G=1)
    assert ints(only["group_of"]) == [0, 1, 1, 2, 3] and only["stats"]["mixed_groups"] == 0


def test_contract_two_rows_with_no_unit_in_common_stay_apart():
    units = [b"XXXABXXX", b"YYYCDYYY", b"ZZZABZZZ", b"WWWCDWWW"]
    got = gu.expected_groups(units, [1, 1, 1, 1], ks=(2,), trim=(3, 3), selected=sel("AB", "CD"), G=1)
    assert ints(got["group_of"]) == [0, 1, 0, 1] and ints(got["head"]) == [0, 1] and got["stats"]["global_edges"] == 0


def test_contract_no_selected_motif_and_no_distance():
    units = [b"CASSLGYEF", b"CASSLGYEW", b"CASSLGYE*", b"", b"A" * 33]
    none = gu.expected_groups(units, [1] * 5, selected=[], G=1)
    assert ints(none["mem_off"]) == [0] and none["need"] == 0
    assert ints(none["group_of"]) == [0, 0, 0, 1, 2] and ints(none["degree"]) == [2, 2, 2, 0, 0]      # a non-letter is linked all the same
    assert none["stats"]["take_part"] == 2 and none["stats"]["global_edges"] == 3
    apart = gu.expected_groups(units, [1] * 5, ks=(2,), trim=(3, 3), selected=sel("SL"), G=0)
    assert ints(apart["group_of"]) == [0, 0, 1, 2, 3] and ints(apart["degree"]) == [0] * 5 and ints(apart["mem"]) == [0, 1]
    alone = gu.expected_groups(units, [1] * 5, selected=[], G=0)
    assert ints(alone["group_of"]) == [0, 1, 2, 3, 4] and alone["stats"]["singleton_groups"] == 5


def test_contract_refuses_selected_motifs_out_of_order_or_outside_k():
    units = [b"XXXABXXX"]
    for bad in ([(2, 5), (2, 5)], [(2, 5), (2, 4)], [(3, 0), (2, 0)], [(5, 0)], [(2, 26 * 26)]):
        with pytest.raises(gu.Invalid):
            gu.expected_groups(units, [1], selected=bad)
    with pytest.raises(gu.Invalid):
        gu.expected_groups(units, [1], ks=(2,), selected=[(3, 0)])
    with pytest.raises(gu.Invalid):
        gu.expected_groups(units, [1], G=3)


# ---- the selection rule ----

def _result(rows):
    """A motifs result of the rows (cs, ge, sum)."""
    return {"k": np.full(len(rows), 2, np.uint32), "code": np.arange(len(rows), dtype=np.uint32), "cs": np.array([r[0] for r in rows], np.uint32),
            "ge": np.array([r[1] for r in rows], np.uint32), "sum": np.array([r[2] for r in rows], np.uint64)}


def test_selection_rule_on_hand_values():
    pick = lambda rows, R, p, fold: motifs.selected_rows(_result(rows), R, Fraction(p), Fraction(fold))
    # p exactly at the threshold: (ge + 1) / (R + 1) = 1 / 1000 at R = 999, ge = 0; one resample more and it is below, one hit more and above
    assert pick([(5, 0, 0)], 999, "0.001", "0") == [0]
    assert pick([(5, 1, 0)], 999, "0.001", "0") == []
    assert pick([(5, 1, 0)], 1999, "0.001", "0") == [0]
    # R = 1000: 1 / 1001 <= 0.001 and 2 / 1001 > 0.001, so ge = 0 alone passes
    assert pick([(5, 0, 0), (5, 1, 0), (5, 2, 0)], 1000, "0.001", "0") == [0]
    # a zero sum passes whatever the fold
    assert pick([(1, 0, 0)], 1000, "0.001", "1000000") == [0]
    # fold exactly at the threshold: cs R = fold sum — 3 * 1000 = 10 * 300; one more in the sum and it fails
    assert pick([(3, 0, 300), (3, 0, 301), (3, 0, 299)], 1000, "0.001", "10") == [0, 2]
    assert pick([(3, 0, 1200)], 1000, "1", "2.5") == [0] and pick([(3, 0, 1201)], 1000, "1", "2.5") == []
    assert pick([(3, 999, 0)], 1000, "1", "0") == [0] and pick([(3, 1000, 0)], 1000, "1.0", "0") == [0]
    # the text is taken exactly: 0.1 is a tenth, not the nearest double
    assert pick([(1, 0, 0)], 9, "0.1", "0") == [0] and pick([(1, 0, 0)], 9, "0.0999999999999999999", "0") == []
    for rows, R, p, fold in (([(3, 0, 300), (4, 2, 1), (1, 0, 0)], 1000, "0.001", "10"), ([(7, 3, 90), (2, 9, 4000)], 50, "0.08", "3.5")):
        assert pick(rows, R, p, fold) == gu.selected_rows(_result(rows), R, p, fold)


def test_decimals():
    assert motifs.parse_decimal("0.001") == Fraction(1, 1000) and motifs.parse_decimal("10") == 10 and motifs.parse_decimal(".5") == Fraction(1, 2)
    assert motifs.parse_decimal("1.") == 1 and motifs.parse_decimal(" 2.50 ") == Fraction(5, 2)
    for bad in ("", "-1", "1e-3", "nan", "inf", "1/2", "0x1", "1,5", ".", "+1"):
        assert motifs.parse_decimal(bad) is None, bad


# ---- the stage, the native calls replaced by the contract ----

G_SAMPLE = [b"CASABCDYEF", b"CASABCEYEF", b"CASQBCDYEF", b"CAS*BCDYEF", b"CASWWWWYEF", b"CASWWWKYEF", b"CASKLMNYEFCASKLMNYEFCASKLMNYEFXXX",
            b"CASPBCPBCF"]
G_BACKGROUND = [b"CASKLMNYEF", b"CASQWCKYEF", b"CASKLVVYEF", b"casklbcyef", b"CASHHHHYEF", b"CASGGGGYEF", b"CASTTTTYEF", b"CASRRRRYEF",
                b"CASNNNNYEF"]
GROUPS_HEAD = "junction_aa\tclonotypes\tduplicate_count\tgroup\tgroup_cdr3s\tgroup_duplicate_count\tdegree\tmotifs"
MEMBERS_HEAD = "motif\tk\tjunction_aa\tposition\tgroup"


@pytest.fixture
def gstage(tmp_path, monkeypatch):
    monkeypatch.setattr(nat, "cdr3_motifs", mu.native_stand_in)
    monkeypatch.setattr(nat, "cdr3_motif_groups", gu.native_stand_in)
    g, bg = str(tmp_path / "G.clonotypes.tsv"), str(tmp_path / "naive.clonotypes.tsv")
    mu.clonotype_file(g, G_SAMPLE, repeat_first=2)      # the first two CDR3s on two rows each: 1 + 2 reads
    mu.clonotype_file(bg, G_BACKGROUND)
    return {"g": g, "bg": bg, "dir": str(tmp_path) + os.sep}


def _gargs(gstage, *more):
    return ["motifs", "-in", gstage["g"], "-bg", gstage["bg"], "-op", gstage["dir"], "-dz", "--motif-min-count", "2", "--motif-k", "2,3",
            "--resamples", "20", "--groups"] + list(more)


def test_stage_both_files_byte_for_byte(gstage, capsys):
    """Under k 2,3 and trim 3,3 a CDR3 of ten letters shows its letters 3 .. 6.  BC is in four of the sample's CDR3s (the last
    one holds it twice, at 4 and at 7, and only the first lies in a window); AB, CD, ABC, BCD, WW and WWW are in two each, and
    no background CDR3 that takes part holds any of them.  So ge = 0 and sum = 0 everywhere: p_value 1/21, and with
    --group-p-value 0.05 all seven are selected.  By distance: ABCD - ABCE, ABCD - QBCD, ABCD - *BCD, QBCD - *BCD, WWWW - WWWK."""
    want = mu.expected_motifs(G_SAMPLE, G_BACKGROUND, (2, 3), (3, 3), 2, 20)
    assert dict(zip(want["letters"], ints(want["cs"]))) == {"AB": 2, "BC": 4, "CD": 2, "WW": 2, "ABC": 2, "BCD": 2, "WWW": 2}
    assert ints(want["ge"]) == [0] * 7 == ints(want["sum"])
    pipeline.main(_gargs(gstage, "--group-p-value", "0.05", "--write-motif-members"))
    text = open(gstage["dir"] + "dcr_G.cdr3_groups.tsv", "rb").read().decode()
    assert text == GROUPS_HEAD + "\n" + "".join(line + "\n" for line in [
        "CASABCDYEF\t2\t3\t0\t5\t9\t3\tAB,BC,CD,ABC,BCD",
        "CASABCEYEF\t2\t3\t0\t5\t9\t1\tAB,BC,ABC",
        "CASQBCDYEF\t1\t1\t0\t5\t9\t2\tBC,CD,BCD",
        "CAS*BCDYEF\t1\t1\t0\t5\t9\t2\t.",
        "CASWWWWYEF\t1\t1\t1\t2\t2\t1\tWW,WWW",
        "CASWWWKYEF\t1\t1\t1\t2\t2\t1\tWW,WWW",
        "CASKLMNYEFCASKLMNYEFCASKLMNYEFXXX\t1\t1\t2\t1\t1\t0\t.",
        "CASPBCPBCF\t1\t1\t0\t5\t9\t0\tBC"])
    members = open(gstage["dir"] + "dcr_G.cdr3_motif_members.tsv", "rb").read().decode()
    assert members == MEMBERS_HEAD + "\n" + "".join(line + "\n" for line in [
        "AB\t2\tCASABCDYEF\t3\t0", "AB\t2\tCASABCEYEF\t3\t0",
        "BC\t2\tCASABCDYEF\t4\t0", "BC\t2\tCASABCEYEF\t4\t0", "BC\t2\tCASQBCDYEF\t4\t0", "BC\t2\tCASPBCPBCF\t4\t0",
        "CD\t2\tCASABCDYEF\t5\t0", "CD\t2\tCASQBCDYEF\t5\t0",
        "WW\t2\tCASWWWWYEF\t3\t1", "WW\t2\tCASWWWKYEF\t3\t1",
        "ABC\t3\tCASABCDYEF\t3\t0", "ABC\t3\tCASABCEYEF\t3\t0",
        "BCD\t3\tCASABCDYEF\t4\t0", "BCD\t3\tCASQBCDYEF\t4\t0",
        "WWW\t3\tCASWWWWYEF\t3\t1", "WWW\t3\tCASWWWKYEF\t3\t1"])
    line = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Groups of G ")]
    assert line == ["Groups of G (motifs with p_value <= 0.05 and fold >= 10, distance 1): 8 CDR3s, 6 take part; 7 motifs selected, "
                    "16 motif members; 5 links by distance; 3 groups (1 of one CDR3, the largest of 5, 2 with both kinds of link)"]
    assert os.path.exists(gstage["dir"] + "dcr_G.cdr3_motifs.tsv")


def test_stage_follows_the_contract_lines_orders_and_the_dot(gstage):
    """The default thresholds at R = 20 select nothing (1/21 > 0.001): every CDR3 has `.`, and the groups are the distance's
    alone; then thresholds that select, compared with the texts written a second time in the util."""
    pipeline.main(_gargs(gstage))
    lines = open(gstage["dir"] + "dcr_G.cdr3_groups.tsv").read().split("\n")
    assert lines[0] == GROUPS_HEAD and lines[-1] == "" and all(x.endswith("\t.") for x in lines[1:-1]) and len(lines) == 10
    assert [x.split("\t")[3] for x in lines[1:-1]] == ["0", "0", "0", "0", "1", "1", "2", "3"]
    assert not os.path.exists(gstage["dir"] + "dcr_G.cdr3_motif_members.tsv")
    for more, G in ((["--group-p-value", "0.05", "--group-min-fold", "0", "--group-distance", "0"], 0),
                    (["--group-p-value", "1", "--group-distance", "2"], 2)):
        out = motifs.run(dict(infile=[gstage["g"]], background=gstage["bg"], outpath=gstage["dir"], prefix="x_", dontgzip=True, motif_min_count=2,
                              motif_k="2,3", resamples=20, groups=True, group_p_value=more[1], group_min_fold="0", group_distance=G,
                              write_motif_members=True))
        result = out["results"][0]
        chosen = gu.selected_rows(result, 20, more[1], "0")
        selected = [(int(result["k"][r]), int(result["code"][r])) for r in chosen]
        assert selected == out["groups"][0]["selected"] and len(selected) == 7
        units = motifs.units_of(G_SAMPLE)
        rows_of, reads_of = [2, 2, 1, 1, 1, 1, 1, 1], [3, 3, 1, 1, 1, 1, 1, 1]
        want = gu.expected_groups(units, reads_of, (2, 3), (3, 3), selected, G)
        got = open(out["groups"][0]["files"]["groups"]).read().split("\n")
        assert got[0] == GROUPS_HEAD and got[-1] == "" and got[1:-1] == gu.groups_lines(units, rows_of, reads_of, want, selected)
        got = open(out["groups"][0]["files"]["members"]).read().split("\n")
        assert got[0] == MEMBERS_HEAD and got[-1] == "" and got[1:-1] == gu.member_lines(units, want, selected, (3, 3))
        keys = [(gu.motif_number(int(f[1]), mu.code_of(f[0].encode())), units.index(f[2].encode())) for f in (x.split("\t") for x in got[1:-1])]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_stage_gzip(gstage):
    args = [a for a in _gargs(gstage, "--group-p-value", "0.05", "--write-motif-members") if a != "-dz"]
    pipeline.main(args)
    pipeline.main(args + ["-dz"])
    for name in ("dcr_G.cdr3_groups.tsv", "dcr_G.cdr3_motif_members.tsv", "dcr_G.cdr3_motifs.tsv"):
        assert gzip.open(gstage["dir"] + name + ".gz", "rb").read() == open(gstage["dir"] + name, "rb").read()


def test_stage_refusals(gstage, capsys, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(nat, "cdr3_motifs", never)
    monkeypatch.setattr(nat, "cdr3_motif_groups", never)
    plain = [a for a in _gargs(gstage) if a != "--groups"]
    for flags, words in ((["--group-p-value", "0.01"], "--group-p-value belongs to --groups"), (["--group-min-fold", "2"], "--group-min-fold belongs"),
                         (["--group-distance", "0"], "--group-distance belongs"), (["--group-distance", "1"], "--group-distance belongs"),
                         (["--write-motif-members"], "--write-motif-members belongs")):
        assert words in cpu._refused(plain + flags, capsys), flags
    groups_r0 = [a if a != "20" else "0" for a in _gargs(gstage)]
    assert "--resamples 0" in cpu._refused(groups_r0, capsys)
    for flags, words in ((["--group-p-value", "0"], "--group-p-value"), (["--group-p-value", "1.5"], "--group-p-value"),
                         (["--group-p-value", "1e-3"], "--group-p-value"), (["--group-p-value", "-0.1"], "--group-p-value"),
                         (["--group-p-value", "x"], "--group-p-value"), (["--group-min-fold", "-1"], "--group-min-fold"),
                         (["--group-min-fold", "ten"], "--group-min-fold"), (["--group-min-fold", "1e1"], "--group-min-fold"),
                         (["--group-distance", "3"], "--group-distance"), (["--group-distance", "-1"], "--group-distance")):
        assert words in cpu._refused(_gargs(gstage, *flags), capsys), flags
    # decided before any file is opened
    base = {"infile": ["nowhere.clonotypes.tsv"], "background": "nowhere.tsv"}
    assert motifs.refusal(dict(base, groups=True)) is None and motifs.refusal(dict(base, groups=True, group_p_value="1", group_min_fold="0")) is None
    assert "--group-p-value" in motifs.refusal(dict(base, group_p_value="0.5"))
    assert "--resamples 0" in motifs.refusal(dict(base, groups=True, resamples=0))
    assert "--group-min-fold" in motifs.refusal(dict(base, groups=True, group_min_fold="-2"))
    assert motifs.refusal(dict(base, write_motif_members=False, groups=False)) is None


def test_without_groups_a_run_writes_what_it_wrote_before(stage, capsys):      # noqa: F811
    """test_motifs' own stage and its own byte-for-byte run: the same file, the same printed lines, and no file more."""
    def never(*a, **k):
        raise AssertionError("the groups were reached")
    import unittest.mock as mock
    with mock.patch.object(nat, "cdr3_motif_groups", never):
        pipeline.main(cpu._args(stage, "--resamples", "0", "--motif-min-count", "2"))
    assert open(stage["dir"] + "dcr_A.cdr3_motifs.tsv", "rb").read().decode() == cpu.HEAD + "\n" + "".join(line + "\n" for line in [
        "BC\t2\t3\t3\t0\t0\t0\t0\tnan\tnan\t1.000000", "AB\t2\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000", "CD\t2\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000",
        "ABC\t3\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000", "BCD\t3\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000"])
    out = capsys.readouterr().out.splitlines()
    assert [x.split(" ")[0] for x in out if x.startswith(("Motifs of", "Groups of"))] == ["Motifs", "Motifs"]
    assert out[[x.startswith("Motifs of A ") for x in out].index(True)] == (
        "Motifs of A against 6 background CDR3s (k 2,3,4, trim 3,3, at least 2): 5 CDR3s, 3 take part (1 out of reach, 1 left "
        "out for a byte outside A..Z); 5 background CDR3s take part (0 out of reach, 1 left out for a byte outside A..Z); "
        "12 distinct motifs, 5 reported; 0 resamples, seed 1")
    written = sorted(x for x in os.listdir(stage["dir"]) if x.startswith("dcr_"))
    assert written == ["dcr_A.cdr3_motifs.tsv", "dcr_B.cdr3_motifs.tsv"]
    res = motifs.run({"infile": [stage["a"]], "background": stage["bg"], "outpath": stage["dir"], "prefix": "q_", "dontgzip": True, "resamples": 3})
    assert sorted(res) == ["motifs", "results", "stats"]


# ---- help, exports, the host program ----

def test_help_names_the_new_flags_and_the_pinned_helps_are_unchanged():
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    got = {c: subprocess.run([sys.executable, "-m", "decombinator_amd", c, "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
           for c in ("motifs", "decombine", "pipeline", "translate")}
    assert got["motifs"].returncode == 0
    for flag in ("--groups", "--group-p-value", "--group-min-fold", "--group-distance", "--write-motif-members", "--resamples", "-bg"):
        assert flag in got["motifs"].stdout, flag
    for command in ("decombine", "pipeline", "translate"):
        with open(os.path.join(cpu.HELP_DIR, command + ".txt")) as fh:
            assert " ".join(got[command].stdout.split()) == " ".join(fh.read().split()), command


def test_exports():
    import ctypes
    names = ("dcrx_cdr3_motif_members_device", "dcrx_cdr3_groups_device", "dcrx_cdr3_motif_groups", "dcrx_cdr3_motif_members_work_bytes",
             "dcrx_cdr3_groups_work_bytes")
    header = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    for name in names:
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", header)
        assert hasattr(nat.lib(), name)
    assert nat.lib().dcrx_abi_version() == 5
    assert ctypes.sizeof(nat.Cdr3MotifGroupStatsC) == 8 * len(nat.CDR3_MOTIF_GROUP_STATS)
    fields = re.search(r"typedef struct dcrx_cdr3_motif_group_stats \{(.*?)\}", header, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == nat.CDR3_MOTIF_GROUP_STATS
    assert nat.CDR3_MOTIF_COUNT == mu.constant("MOTIFS")
    assert callable(nat.cdr3_motif_members) and callable(nat.cdr3_motif_groups)
    # the work-space sizes are answered on the host: what is refused is 0
    assert nat.cdr3_motif_members_work_bytes(1 << 30, 0) == 0 and nat.cdr3_motif_members_work_bytes(1 << 29, (1 << 31) - (1 << 29)) == 0
    assert nat.cdr3_groups_work_bytes(1 << 30, 0) == 0 and nat.cdr3_groups_work_bytes(10, nat.CDR3_MOTIF_COUNT + 1) == 0


def test_host_program_of_the_shared_header_plain_and_under_sanitizers():
    """The selected motifs' order check and the sort's constants: a stand-alone program (its own main), on the CPU."""
    plain = gu.host_program()
    got = subprocess.run([plain], capture_output=True, text=True)
    assert got.returncode == 0 and got.stdout.strip().endswith("ok"), got.stdout + got.stderr
    for words, want in ((["0x1c", "2:0", "2:5", "3:1", "4:7"], 4), (["0x1c", "2:0", "2:5", "3:1", "2:7"], 3), (["0x1c", "2:5", "2:5"], 1),
                        (["0x0c", "2:0", "4:0"], 1), (["0x1c", "2:676"], 0), (["0x1c"], 0)):
        assert int(subprocess.run([plain] + words, capture_output=True, text=True).stdout) == want, words
        k, code = [int(w.split(":")[0]) for w in words[1:]], [int(w.split(":")[1]) for w in words[1:]]
        try:
            gu.check_selected(list(zip(k, code)), [x for x in (2, 3, 4) if int(words[0], 16) >> x & 1])
            assert want == len(k)
        except gu.Invalid:
            assert want < len(k)
    got = subprocess.run(["make", "-s", "-C", gu.HOST_DIR, "asan"], capture_output=True, text=True)
    assert got.returncode == 0 and got.stdout.strip().endswith("ok"), got.stdout[-2000:] + got.stderr[-2000:]
