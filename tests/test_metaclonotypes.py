"""The `metaclonotypes` sub-command without a GPU: the radius rule on hand values, the stage with the native calls replaced by the
contract (tests/cdr3_profile_util.py, tests/cdr3_wmatch_util.py) against files written by hand, every refusal, the help texts."""
import gzip
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import metaclonotypes as mc
from decombinator_amd import pipeline
from tests import cdr3_match_util as mu
from tests import cdr3_profile_util as pu
from tests import cdr3_wmatch_util as wu
from tests.test_cdr3_match import clonotypes_text
from tests.test_motifs import HELP_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the radius rule ----

def test_radius_rule_on_hand_values():
    rate = mc.parse_rate("1e-5")
    assert rate == Fraction(1, 100000) == mc.parse_rate("1/100000") == mc.parse_rate("0.00001") == mc.parse_rate(" 1E-5 ")
    M = 300000      # the threshold: B * 100000 <= 300000, so B <= 3
    rows = [[0, 0, 3, 3, 4], [0, 1, 2, 3, 3], [4, 4, 4, 4, 4], [3, 4, 5, 6, 7], [0, 0, 0, 0, 0]]
    assert mc.radius_bins(rows, M, rate).tolist() == [3, 4, -1, 0, 4]      # exactly at the threshold passes, one above does not
    assert mc.radius_bins(rows, M - 1, rate).tolist() == [1, 2, -1, -1, 4]      # 299999 / 100000: B <= 2
    # rate 0: the last r with B = 0; rate 1: everything passes while B <= M
    assert mc.radius_bins(rows, M, Fraction(0)).tolist() == [1, 0, -1, -1, 4]
    assert mc.radius_bins(rows, 5, Fraction(1)).tolist() == [4, 4, 4, 2, 4]
    # M = 0: only B = 0 passes, whatever the rate
    assert mc.radius_bins(rows, 0, Fraction(1)).tolist() == [1, 0, -1, -1, 4]
    assert mc.radius_bins(np.zeros((0, 5), np.uint64), 7, rate).tolist() == []
    # a denominator far past 64 bits stays exact
    assert mc.radius_bins([[1, 2, 3]], 10 ** 30, Fraction(2, 10 ** 30)).tolist() == [1]


def test_rates_that_are_refused():
    for bad in ("-1e-5", "1.0000001", "2", "x", "", "1/0", "1e", "1e-5x", "nan", "inf"):
        assert mc.parse_rate(bad) is None, bad
    assert mc.parse_rate("0") == 0 and mc.parse_rate("1") == 1 and mc.parse_rate("1/3") == Fraction(1, 3)


# ---- the stage, with the contract in the native calls' place ----

A_ROWS = [("TRBV1*01", "TRBJ1*01", "CASSIRSSYEQYF", 10),      # 0: the background holds CASSLRSSYEQYF at 6 and CASSWRSSYEQYF at 12
          ("TRBV1*01", "TRBJ1*01", "CASSVRSSYEQYF", 5),       # 1: I-V 3 from clonotype 0
          ("TRBV1*01", "TRBJ1*01", "CASSIRSYEQYF", 3),        # 2: one residue less: 12 from clonotype 0
          ("TRBV1*01", "TRBJ1*01", "CASSIRSS*EQYF", 2),       # 3: takes no part
          ("TRBV2*01", "TRBJ1*01", "CASSIRSSYEQYF", 1),       # 4: another V: the background holds the same CDR3 under TRBV2
          ("TRBV1*02", "TRBJ1*01", "CASSIRSSYEQYF", 7)]       # 5: another allele: a class of its own unless --strip-alleles
BG = (b"CDR3\tV\tJ\n"
      b"CASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\n"
      b"CASSWRSSYEQYF\tTRBV1*01\tTRBJ1*01\n"
      b"CASSIRSSYEQYF\tTRBV2*01\tTRBJ1*01\n"
      b"CASS_RSSYEQYF\tTRBV1*01\tTRBJ1*01\n"
      b"CASSIRSSYEQYF\tTRBV9*01\tTRBJ1*01\n")
BG_FLAGS = dict(bg_cdr3_column="CDR3", bg_v_column="V", bg_j_column="J")
HEAD = b"clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\tradius\tbackground_neighbours\tbackground\tsample_neighbours\n"


def write_inputs(tmp_path, tables, bg=BG, bg_name="bg.tsv"):
    files = []
    for name, rows in tables:
        path = str(tmp_path / (name + ".clonotypes.tsv"))
        with open(path, "wb") as fh:
            fh.write(clonotypes_text(rows))
        files.append(path)
    bg_path = str(tmp_path / bg_name)
    with open(bg_path, "wb") as fh:
        fh.write(bg)
    return files, bg_path


def stage(tmp_path, monkeypatch, files, bg_path, calls=None, matches=None, **kw):
    mu.StubIndex.made.clear()
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_profile_weighted", pu.brute_force_native(calls))
    monkeypatch.setattr(nat, "cdr3_match_weighted", wu.brute_force_native(matches))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out, exist_ok=True)
    inp = dict(command="metaclonotypes", infile=files, background=bg_path, outpath=out, prefix="t_", dontgzip=True, **BG_FLAGS)
    inp.update(kw)
    return mc.run(inp), out


def test_the_three_files_byte_for_byte(tmp_path, monkeypatch, capsys):
    files, bg = write_inputs(tmp_path, [("A", A_ROWS)])
    calls, matches = [], []
    # M = 4 background CDR3s take part; rate 1/4: one background neighbour passes, two do not
    res, out = stage(tmp_path, monkeypatch, files, bg, calls, matches, cdr3_radius=12, radius_step=3, max_background_rate="1/4",
                     write_radius_profile=True, write_metaclonotype_members=True)
    # clonotype 0: background at 6 (I-L) and 12 (I-W): B = 0 0 1 1 2 over r = 0 3 6 9 12 -> radius 9; the sample within 9: itself and 1
    # clonotype 1: V-L 9, V-W 12: B = 0 0 0 1 2 -> radius 9; the sample within 9: itself and 0
    # clonotype 2: 12 + I-L 6 = 18, beyond the ladder: B = 0 -> radius 12; the sample within 12: itself and 0 (1 is at 15)
    # clonotype 4: the background holds its CDR3 under its V at 0: B(0) = 1 <= 1 -> radius 12, nobody of its class in the sample
    # clonotype 5: TRBV1*02 is a class the background lacks: radius 12, alone
    assert open(res["metaclonotypes"][0], "rb").read() == HEAD + (
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t9\t1\t4\t1\n"
        b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t5\t9\t1\t4\t1\n"
        b"2\tTRBV1*01\tTRBJ1*01\tCASSIRSYEQYF\t3\t12\t0\t4\t1\n"
        b"4\tTRBV2*01\tTRBJ1*01\tCASSIRSSYEQYF\t1\t12\t1\t4\t0\n"
        b"5\tTRBV1*02\tTRBJ1*01\tCASSIRSSYEQYF\t7\t12\t0\t4\t0\n")
    assert open(res["profiles"][0], "rb").read() == (
        b"clonotype\tbg_le_0\tbg_le_3\tbg_le_6\tbg_le_9\tbg_le_12\ts_le_0\ts_le_3\ts_le_6\ts_le_9\ts_le_12\n"
        b"0\t0\t0\t1\t1\t2\t1\t2\t2\t2\t3\n"
        b"1\t0\t0\t0\t1\t2\t1\t2\t2\t2\t2\n"
        b"2\t0\t0\t0\t0\t0\t1\t1\t1\t1\t2\n"
        b"4\t1\t1\t1\t1\t1\t1\t1\t1\t1\t1\n"
        b"5\t0\t0\t0\t0\t0\t1\t1\t1\t1\t1\n")
    assert open(res["members"][0], "rb").read() == (
        b"clonotype\tradius\tmember\tmember_junction_aa\tmember_duplicate_count\tdistance\n"
        b"0\t9\t1\tCASSVRSSYEQYF\t5\t3\n"
        b"1\t9\t0\tCASSIRSSYEQYF\t10\t3\n"
        b"2\t12\t0\tCASSIRSSYEQYF\t10\t12\n")
    assert [os.path.basename(x) for x in res["metaclonotypes"] + res["profiles"] + res["members"]] == [
        "t_A.cdr3_metaclonotypes.tsv", "t_A.cdr3_radius_profile.tsv", "t_A.cdr3_metaclonotype_members.tsv"]
    # two profile calls (the background's index, the sample's own), one match at the sample's largest radius
    assert [(c[0] is mu.StubIndex.made[0], c[4], c[5]) for c in calls] == [(True, 3, 5), (False, 3, 5)]
    assert len(matches) == 1 and matches[0][5] == 12 and matches[0][0] is mu.StubIndex.made[1]
    assert len(mu.StubIndex.made) == 2 and all(x.closed for x in mu.StubIndex.made)
    assert mu.StubIndex.made[1].strings == [r[2].encode() for r in A_ROWS]
    assert capsys.readouterr().out.splitlines()[0] == (
        "Meta-clonotypes of A against 4 background CDR3s (radii 0 to 12 by 3, at most 1/4 of the background, gap 12, trim 3,2, class v): "
        "6 clonotypes, 5 take part (1 left out for a byte outside A..Z, 0 out of reach), 5 with a radius, 3 of them with a sample neighbour")
    assert mc.stats["A"] == {"clonotypes": 6, "take_part": 5, "not_letters": 1, "out_of_reach": 0, "background": 5, "background_take_part": 4,
                             "with_radius": 5, "with_neighbours": 3}


def test_no_radius_is_a_dot_and_rate_0(tmp_path, monkeypatch):
    files, bg = write_inputs(tmp_path, [("A", A_ROWS)])
    res, _ = stage(tmp_path, monkeypatch, files, bg, cdr3_radius=12, radius_step=3, max_background_rate="0",
                   write_metaclonotype_members=True)
    # rate 0: the last r with B = 0; clonotype 4 meets the background at 0 and has none
    assert open(res["metaclonotypes"][0], "rb").read() == HEAD + (
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t3\t0\t4\t1\n"
        b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t5\t6\t0\t4\t1\n"
        b"2\tTRBV1*01\tTRBJ1*01\tCASSIRSYEQYF\t3\t12\t0\t4\t1\n"
        b"4\tTRBV2*01\tTRBJ1*01\tCASSIRSSYEQYF\t1\t.\t.\t4\t.\n"
        b"5\tTRBV1*02\tTRBJ1*01\tCASSIRSSYEQYF\t7\t12\t0\t4\t0\n")
    assert open(res["members"][0], "rb").read().splitlines()[1:] == [
        b"0\t3\t1\tCASSVRSSYEQYF\t5\t3", b"1\t6\t0\tCASSIRSSYEQYF\t10\t3", b"2\t12\t0\tCASSIRSSYEQYF\t10\t12"]
    assert res["profiles"] == [] and mc.stats["A"]["with_radius"] == 4


def test_strip_alleles_two_samples_gzip_and_defaults(tmp_path, monkeypatch, capsys):
    b_rows = [("TRBV9*01", "TRBJ1*01", "CASSIRSSYEQYF", 4), ("TRBV9*01", "TRBJ1*01", "", 1), ("TRBV9*01", "TRBJ1*01", "A" * 33, 1)]
    files, bg = write_inputs(tmp_path, [("A", A_ROWS), ("B", b_rows)])
    calls = []
    res, out = stage(tmp_path, monkeypatch, files, bg, calls, strip_alleles=True, dontgzip=False, write_radius_profile=True)
    assert [os.path.basename(x) for x in res["metaclonotypes"]] == ["t_A.cdr3_metaclonotypes.tsv.gz", "t_B.cdr3_metaclonotypes.tsv.gz"]
    assert [os.path.basename(x) for x in res["profiles"]] == ["t_A.cdr3_radius_profile.tsv.gz", "t_B.cdr3_radius_profile.tsv.gz"]
    assert [(c[4], c[5]) for c in calls] == [(2, 25)] * 4 and (calls[0][3].gap, calls[0][3].ntrim, calls[0][3].ctrim) == (12, 3, 2)
    a = gzip.open(res["metaclonotypes"][0], "rb").read().splitlines()
    # TRBV1*01 and TRBV1*02 are one class now: clonotypes 0 and 5 are each other's neighbours at 0.  Rate 1e-5 of M = 4: B = 0 alone
    assert a[1] == b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t4\t0\t4\t2" and a[5] == b"5\tTRBV1*02\tTRBJ1*01\tCASSIRSSYEQYF\t7\t4\t0\t4\t2"
    assert a[4] == b"4\tTRBV2*01\tTRBJ1*01\tCASSIRSSYEQYF\t1\t.\t.\t4\t."
    b = gzip.open(res["metaclonotypes"][1], "rb").read().splitlines()
    assert b == [HEAD[:-1], b"0\tTRBV9*01\tTRBJ1*01\tCASSIRSSYEQYF\t4\t.\t.\t4\t."]
    assert len(gzip.open(res["profiles"][0], "rb").read().splitlines()[0].split(b"\t")) == 1 + 2 * 25
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Meta-clonotypes of")]
    assert lines[1].endswith("3 clonotypes, 1 take part (0 left out for a byte outside A..Z, 2 out of reach), 0 with a radius, "
                             "0 of them with a sample neighbour")
    assert "radii 0 to 48 by 2, at most 1/100000 of the background" in lines[0]
    # classes are numbered over the background and all samples: B's TRBV9 is the background's fifth entry's class
    assert calls[2][1][0] == mu.StubIndex.made[0].classes[4]


def test_a_background_with_nothing_within_the_ladder_gives_the_top(tmp_path, monkeypatch):
    far = b"CDR3\tV\tJ\nWWWWWWWWWWWWW\tTRBV1*01\tTRBJ1*01\n"
    files, bg = write_inputs(tmp_path, [("A", A_ROWS[:2])], bg=far)
    res, _ = stage(tmp_path, monkeypatch, files, bg, cdr3_radius=24, radius_step=12)
    assert open(res["metaclonotypes"][0], "rb").read().splitlines()[1:] == [
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t24\t0\t1\t1", b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t5\t24\t0\t1\t1"]


# ---- refusals ----

def _no_open(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a file was opened, or the device called, before the refusal")
    monkeypatch.setattr(mc, "read_table", boom)
    monkeypatch.setattr(mc, "read_database", boom)
    for name in ("Cdr3Index", "cdr3_profile_weighted", "cdr3_match_weighted"):
        monkeypatch.setattr(nat, name, boom)
    monkeypatch.setattr(nat.Cdr3Cost, "from_file", boom)


@pytest.mark.parametrize("kw,msg", [
    ({"infile": []}, "1 to 64"),
    ({"infile": [f"s{k}.clonotypes.tsv" for k in range(65)]}, "1 to 64"),
    ({"infile": ["x/a.clonotypes.tsv", "y/a.clonotypes.tsv.gz"]}, "one sample name"),
    ({"background": None}, "takes a background"),
    ({"cdr3_radius": 49}, "multiple of --radius-step"),
    ({"cdr3_radius": 10, "radius_step": 3}, "multiple of --radius-step"),
    ({"cdr3_radius": 64}, "more than 32"),
    ({"cdr3_radius": 32, "radius_step": 1}, "more than 32"),
    ({"radius_step": 0}, "--radius-step is 1 to 65535"),
    ({"radius_step": 65536, "cdr3_radius": 0}, "--radius-step is 1 to 65535"),
    ({"cdr3_radius": 65536, "radius_step": 4096}, "--cdr3-radius is 0 to 65535"),
    ({"cdr3_radius": -2}, "--cdr3-radius is 0 to 65535"),
    ({"max_background_rate": "1.5"}, "--max-background-rate"),
    ({"max_background_rate": "-1e-5"}, "--max-background-rate"),
    ({"max_background_rate": "few"}, "--max-background-rate"),
    ({"max_background_rate": "1/0"}, "--max-background-rate"),
    ({"cdr3_gap_cost": 0}, "--cdr3-gap-cost is 1 to 255"),
    ({"cdr3_trim": "17,0"}, "--cdr3-trim is N,C"),
    ({"cdr3_class": "j"}, "--cdr3-class is none, v or vj"),
])
def test_refusals_before_anything_is_opened(monkeypatch, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="metaclonotypes", infile=["a.clonotypes.tsv"], background="bg.tsv", outpath="", prefix="", dontgzip=True)
    inp.update(kw)
    assert msg in mc.refusal(inp)
    with pytest.raises(ValueError, match=msg):
        mc.run(inp)


def test_the_limits_pass():
    base = dict(infile=["a.clonotypes.tsv"], background="bg.tsv")
    for kw in ({}, {"cdr3_radius": 62}, {"cdr3_radius": 31, "radius_step": 1}, {"cdr3_radius": 0}, {"cdr3_radius": 65535, "radius_step": 65535},
               {"max_background_rate": "0"}, {"max_background_rate": "1"}, {"max_background_rate": "1/100000"}):
        assert mc.refusal(dict(base, **kw)) is None, kw
    assert mc.ladder(base) == (2, 25) and mc.ladder(dict(base, cdr3_radius=0)) == (2, 1)


def test_a_missing_background_column_is_refused_by_its_flag(tmp_path, monkeypatch):
    files, bg = write_inputs(tmp_path, [("A", A_ROWS)])
    with pytest.raises(ValueError, match=r"no column 'junction_aa' \(--bg-cdr3-column\)"):
        stage(tmp_path, monkeypatch, files, bg, bg_cdr3_column="junction_aa")
    with pytest.raises(ValueError, match=r"no column 'v_call' \(--bg-v-column\)"):
        stage(tmp_path, monkeypatch, files, bg, bg_v_column="v_call")
    res, _ = stage(tmp_path, monkeypatch, files, bg, bg_v_column="v_call", bg_j_column="nope", cdr3_class="none")      # (not needed: not read)
    assert len(res["metaclonotypes"]) == 1


def test_refusals_from_the_command_line_and_the_parser(monkeypatch, capsys):
    from decombinator_amd.io import cli_args
    _no_open(monkeypatch)
    base = ["metaclonotypes", "-in", "a.clonotypes.tsv", "-bg", "bg.tsv"]
    for words, msg in ((base + ["--cdr3-radius", "49"], "multiple of --radius-step"), (base + ["--radius-step", "0"], "--radius-step"),
                       (base + ["--max-background-rate", "3"], "--max-background-rate"), (base[:3], "takes a background")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(words)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    inp = cli_args(base)
    assert inp["command"] == "metaclonotypes" and (inp["cdr3_radius"], inp["radius_step"], inp["max_background_rate"]) == (None, None, None)
    assert (inp["cdr3_class"], inp["strip_alleles"], inp["write_radius_profile"], inp["write_metaclonotype_members"]) == ("v", False, False, False)
    assert mc.refusal(inp) is None
    inp = cli_args(base + ["--cdr3-radius", "36", "--radius-step", "4", "--max-background-rate", "1/100000", "--cdr3-gap-cost", "8",
                           "--cdr3-trim", "4,3", "--cdr3-cost-matrix", "m.tsv", "--bg-v-column", "V", "--write-radius-profile"])
    assert mc.refusal(inp) is None and mc.ladder(inp) == (4, 10) and inp["max_background_rate"] == "1/100000" and inp["bg_v_column"] == "V"


# ---- help ----

def test_help_names_every_flag_and_the_other_helps_are_unchanged():
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    got = {c: subprocess.run([sys.executable, "-m", "decombinator_amd", c, "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
           for c in ("metaclonotypes", "decombine", "pipeline", "translate")}
    assert got["metaclonotypes"].returncode == 0
    for flag in ("-in", "-bg", "-op", "-pf", "-dz", "--cdr3-radius", "--radius-step", "--max-background-rate", "--cdr3-class", "--strip-alleles",
                 "--cdr3-gap-cost", "--cdr3-trim", "--cdr3-cost-matrix", "--bg-cdr3-column", "--bg-v-column", "--bg-j-column",
                 "--write-radius-profile", "--write-metaclonotype-members"):
        assert flag in got["metaclonotypes"].stdout, flag
    assert "not measured optima" in " ".join(got["metaclonotypes"].stdout.split())
    for command in ("decombine", "pipeline", "translate"):
        with open(os.path.join(HELP_DIR, command + ".txt")) as fh:
            assert " ".join(got[command].stdout.split()) == " ".join(fh.read().split()), command
    from decombinator_amd.io import create_parser
    choices = [a.choices for a in create_parser()._actions if getattr(a, "choices", None)]
    assert [list(c) for c in choices] == [["pipeline", "decombine", "collapse", "translate", "overlap"]]
    epilog = create_parser().epilog
    assert "metaclonotypes" in epilog and "motifs" in epilog and "match" in epilog
