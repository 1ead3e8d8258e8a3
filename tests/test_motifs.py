"""`motifs` without a GPU: the shared header through a host build against Python; the contract in Python (mu.expected_motifs)
on hand-made tables whose answers are written out here; the resamples' sanity against the hypergeometric mean and a planted
motif; the stage with the native call replaced by the contract — the file byte for byte, the order of its lines, `nan` at
R = 0, the printed line, gzip, every refusal —; the help texts; the exports."""
import gzip
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import motifs, pipeline
from tests import motif_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELP_DIR = os.path.join(ROOT, "tests", "golden", "overlap_help")


# ---- the shared header ----

def test_window_ranges_for_every_length_trim_and_k():
    h = mu.host_lib()
    for L in range(33):
        for N in range(17):
            for C in range(17):
                for k in (2, 3, 4):
                    windows = [p for p in range(L) if N <= p and p + k <= L - C]
                    assert h.motif_host_window_count(L, N, C, k) == len(windows), (L, N, C, k)
                    assert len(windows) <= mu.constant("MAX_WINDOWS")


def test_motif_order_is_the_order_of_the_letters():
    h = mu.host_lib()
    words = {k: sorted({bytes(w) for w in np.random.default_rng(k).integers(65, 91, size=(300, k), dtype=np.uint8).tolist()}
                       | {b"A" * k, b"Z" * k, b"A" * (k - 1) + b"B", b"B" + b"A" * (k - 1)}) for k in (2, 3, 4)}
    ids = []
    for k in (2, 3, 4):
        for w in words[k]:
            unit = b"QQ" + w + b"Q"
            code = h.motif_host_code_at(unit, len(unit), 2, k)
            assert code == mu.code_of(w) and nat.cdr3_motif_text(k, code) == w.decode()
            mid = h.motif_host_motif_id(k, code)
            assert (h.motif_host_id_k(mid), h.motif_host_id_code(mid)) == (k, code)
            ids.append(mid)
    assert ids == sorted(ids) and len(set(ids)) == len(ids)      # (k, letters) ascending is the number ascending
    assert h.motif_host_motif_id(4, mu.code_of(b"ZZZZ")) == mu.constant("MOTIFS") - 1 == 26 ** 2 + 26 ** 3 + 26 ** 4 - 1
    assert h.motif_host_motif_id(2, 0) == 0


def test_deduplication_in_the_header():
    for k in (2, 3, 4):
        assert mu.host_unit_motifs(b"AAAAAAAAAA", (0, 0), k) == [mu.host_lib().motif_host_motif_id(k, 0)]
    got = mu.host_unit_motifs(b"CASSLGASSLF", (1, 1), 3)      # ASS and SSL twice
    want = []
    for p in range(1, 11 - 1 - 3 + 1):
        w = b"CASSLGASSLF"[p:p + 3]
        if w not in want:
            want.append(w)
    assert [nat.cdr3_motif_text(3, mu.host_lib().motif_host_id_code(i)) for i in got] == [w.decode() for w in want] and len(want) == 5
    for unit in (b"", b"A" * 33, b"CASsF", b"CAS*F"):
        assert mu.host_unit_motifs(unit, (0, 0), 2) is None and not mu.takes_part(unit)
    assert mu.host_unit_motifs(b"CASSF", (3, 3), 2) == []      # too short for a window: it takes part all the same


def test_header_against_the_sets_on_random_units():
    rng = np.random.default_rng(5)
    for unit in mu.random_units(200, 5, 1, 32):
        trim = (int(rng.integers(0, 6)), int(rng.integers(0, 6)))
        for k in (2, 3, 4):
            got = mu.host_unit_motifs(unit, trim, k)
            assert len(got) == len(set(got))
            assert {(k, nat.cdr3_motif_text(k, mu.host_lib().motif_host_id_code(i)).encode()) for i in got} == mu.motif_set(unit, (k,), trim)


def test_selection_digits_and_chunk_rule():
    h = mu.host_lib()
    bits = 64 // mu.constant("LEVELS")
    assert 1 << bits == mu.constant("BINS") == mu.constant("BLOCK")
    key = 0x0123456789ABCDEF
    for level in range(mu.constant("LEVELS")):
        assert h.motif_host_digit(key, level) == key >> (64 - bits * (level + 1)) & (mu.constant("BINS") - 1)
        assert h.motif_host_prefix(key, level) == (key >> (64 - bits * level) if level else 0)
    assert mu.chunk_of(0) == mu.chunk_of(1) == mu.chunk_of(5000) == mu.constant("MAX_CHUNK")
    assert mu.chunk_of(100_000) == (1 << 25) // (mu.constant("MOTIFS") + 100_000)
    assert mu.chunk_of(1 << 29) == 1


# ---- the contract on hand-made tables ----

def _table(result):
    return {(int(k), text): (int(cs), int(cb)) for k, text, cs, cb in zip(result["k"], result["letters"], result["cs"], result["cb"])}


def test_contract_a_motif_twice_in_one_unit_counts_once():
    sample = [b"XXXABABXXX", b"XXXABCCXXX"]
    got = mu.expected_motifs(sample, [b"XXXABABABXXX"], ks=(2,), trim=(3, 3), min_count=1, resamples=0)
    assert _table(got) == {(2, "AB"): (2, 1), (2, "BA"): (1, 1), (2, "BC"): (1, 0), (2, "CC"): (1, 0)}
    assert list(got["letters"]) == ["AB", "BA", "BC", "CC"] and got["need"] == 4


def test_contract_a_motif_in_the_trimmed_ends_is_not_found():
    sample = [b"GTDAAAAGTD", b"GTDAAAAGTD"[::-1]]
    got = mu.expected_motifs(sample, [], ks=(3,), trim=(3, 3), min_count=1, resamples=0)
    assert _table(got) == {(3, "AAA"): (2, 0)}      # GTD lies in the first and the last three alone
    got = mu.expected_motifs(sample, [], ks=(3,), trim=(0, 3), min_count=1, resamples=0)
    assert (3, "GTD") in _table(got) and _table(got)[(3, "GTD")] == (1, 0)


def test_contract_lengths_and_bytes_that_take_no_part():
    long32, long33 = b"CAS" + b"KL" * 13 + b"YEF", b"CAS" + b"KL" * 13 + b"YEFF"
    assert (len(long32), len(long33)) == (32, 33)
    sample = [long32, long33, b"CASkLKLYEF", b"CAS*KLKYEF", b"", b"CASKLKLYEF"]
    got = mu.expected_motifs(sample, [long33, b"CASKLQQYEF", b"casklklyef"], ks=(2,), trim=(3, 3), min_count=1, resamples=0)
    st = got["stats"]
    assert (st["sample_units"], st["sample_take_part"], st["sample_out_of_reach"], st["sample_not_letters"]) == (6, 2, 2, 2)
    assert (st["background_units"], st["background_take_part"], st["background_out_of_reach"], st["background_not_letters"]) == (3, 1, 1, 1)
    assert _table(got) == {(2, "KL"): (2, 1), (2, "LK"): (2, 0)} and st["motifs"] == st["reported"] == 2


def test_contract_one_k_alone_and_min_count_at_the_count():
    sample = [b"XXXABCDXXX", b"XXXABCEXXX", b"XXXQBCDXXX"]
    only3 = mu.expected_motifs(sample, sample, ks=(3,), trim=(3, 3), min_count=1, resamples=0)
    assert _table(only3) == {(3, "ABC"): (2, 2), (3, "BCD"): (2, 2), (3, "BCE"): (1, 1), (3, "QBC"): (1, 1)}
    at = mu.expected_motifs(sample, sample, ks=(2, 3, 4), trim=(3, 3), min_count=3, resamples=0)
    assert _table(at) == {(2, "BC"): (3, 3)} and at["stats"]["motifs"] == 5 + 4 + 3 and at["stats"]["reported"] == 1
    above = mu.expected_motifs(sample, sample, ks=(2, 3, 4), trim=(3, 3), min_count=4, resamples=0)
    assert above["need"] == 0 and len(above["k"]) == 0 and above["stats"]["motifs"] == 12


def test_contract_resamples_on_a_hand_made_background():
    """n' = m': every resample is the whole background, so c_r = cb for every r; n' > m' is refused; R = 0 leaves zeros."""
    units = [b"XXXABXXX", b"XXXABXXX"[:3] + b"CD" + b"XXX", b"XXXABXXY"]
    got = mu.expected_motifs(units, units, ks=(2,), trim=(3, 3), min_count=1, resamples=7, seed=3)
    assert _table(got) == {(2, "AB"): (2, 2), (2, "CD"): (1, 1)}
    assert [int(x) for x in got["ge"]] == [7, 7] and [int(x) for x in got["sum"]] == [14, 7] and [int(x) for x in got["max"]] == [2, 1]
    with pytest.raises(mu.Invalid):
        mu.expected_motifs(units, units[:2], ks=(2,), resamples=1)
    none = mu.expected_motifs(units, units[:2], ks=(2,), min_count=1, resamples=0)
    assert [int(x) for x in none["ge"]] == [0, 0] == [int(x) for x in none["sum"]]
    # n' = 1 of m' = 3: the kept unit is the one with the smallest key, computed here from the key itself
    one = mu.expected_motifs(units[:1], units, ks=(2,), min_count=1, resamples=5, seed=9)
    want = sum(min(range(3), key=lambda b: mu.ru.key(9, r, b)) in (0, 2) for r in range(5))
    assert [int(x) for x in one["sum"]] == [want] and one["kept_counts"] == [1] * 5


# ---- the resamples' sanity ----

def _sanity_tables():
    """2 000 random units of 11 to 17 letters and every tenth of them as the sample.  The table's seed is one under which GTD, TDT
    and GTDT lie in at most two background units each (the planted motif's premise: seen on the table alone, before any result)."""
    background = list(mu.random_units(2000, 12))
    return background[::10], background


def test_resample_means_follow_the_hypergeometric_mean():
    sample, background = _sanity_tables()
    R = 1000
    got = mu.expected_motifs(sample, background, ks=(2,), trim=(3, 3), min_count=3, resamples=R, seed=1)
    n, m = got["stats"]["sample_take_part"], got["stats"]["background_take_part"]
    assert (n, m) == (200, 2000) and got["kept_counts"] == [n] * R
    checked, worst = 0, 0.0
    for cb, total in zip(got["cb"], got["sum"]):
        cb, total = int(cb), int(total)
        if cb < 20:
            continue
        p = cb / m
        se = math.sqrt(n * p * (1 - p) * (m - n) / (m - 1) / R)
        worst = max(worst, abs(total / R - n * cb / m) / se)
        checked += 1
    print(f"{checked} motifs, at most {worst:.2f} standard errors")
    assert checked > 100 and worst <= 6.0


def test_a_planted_motif_stands_out():
    sample, background = _sanity_tables()
    sample = mu.planted(sample, b"GTDT", 4, 30)      # residues 5 .. 8: inside the windows of the shortest unit (11 letters) too
    got = mu.expected_motifs(sample, background, ks=(2, 3, 4), trim=(3, 3), min_count=3, resamples=200, seed=1)
    rows = {text: (int(ge), int(cb), int(cs)) for text, ge, cb, cs in zip(got["letters"], got["ge"], got["cb"], got["cs"])}
    for mo in ("GTDT", "GTD", "TDT"):
        assert mo in rows and rows[mo][0] == 0 and rows[mo][1] <= 2 and rows[mo][2] >= 30, (mo, rows.get(mo))


# ---- the stage, the native call replaced by the contract ----

SAMPLE_A = [b"CASABCDYEF", b"CASABCEYEF", b"CASQBCDYEF", b"CAS*BCDYEF", b"CASABCDYEFCASABCDYEFCASABCDYEFXXX"]
SAMPLE_B = [b"CASBCBCYEF", b"CASKBCKYEF"]
BACKGROUND = [b"CASABCDYEF", b"CASKLMNYEF", b"CASQBCKYEF", b"CASKLBCYEF", b"casklbcyef", b"CASWWWWYEF"]


@pytest.fixture
def stage(tmp_path, monkeypatch):
    monkeypatch.setattr(nat, "cdr3_motifs", mu.native_stand_in)
    a, b, bg = (str(tmp_path / name) for name in ("A.clonotypes.tsv", "B.clonotypes.tsv", "naive.clonotypes.tsv"))
    mu.clonotype_file(a, SAMPLE_A, repeat_first=2)
    mu.clonotype_file(b, SAMPLE_B)
    mu.clonotype_file(bg, BACKGROUND, repeat_first=3)
    return {"a": a, "b": b, "bg": bg, "dir": str(tmp_path) + os.sep}


def _args(stage, *more, files=None):
    return ["motifs", "-in"] + (files or [stage["a"], stage["b"]]) + ["-bg", stage["bg"], "-op", stage["dir"], "-dz"] + list(more)


HEAD = "motif\tk\tcdr3s\tbackground_cdr3s\tresamples\tresamples_at_least\tresample_sum\tresample_max\texpected\tfold\tp_value"


def test_stage_file_byte_for_byte_at_r_0(stage, capsys):
    pipeline.main(_args(stage, "--resamples", "0", "--motif-min-count", "2"))
    text = open(stage["dir"] + "dcr_A.cdr3_motifs.tsv", "rb").read().decode()
    # A's units that take part: ABCD, ABCE, QBCD (a repeated row is one unit).  ge 0 everywhere, so cdr3s descending, then k, then motif
    assert text == HEAD + "\n" + "".join(line + "\n" for line in [
        "BC\t2\t3\t3\t0\t0\t0\t0\tnan\tnan\t1.000000",
        "AB\t2\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000",
        "CD\t2\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000",
        "ABC\t3\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000",
        "BCD\t3\t2\t1\t0\t0\t0\t0\tnan\tnan\t1.000000"])
    out = capsys.readouterr().out
    line = [x for x in out.splitlines() if x.startswith("Motifs of A ")][0]
    assert line == ("Motifs of A against 6 background CDR3s (k 2,3,4, trim 3,3, at least 2): 5 CDR3s, 3 take part (1 out of reach, 1 left "
                    "out for a byte outside A..Z); 5 background CDR3s take part (0 out of reach, 1 left out for a byte outside A..Z); "
                    "12 distinct motifs, 5 reported; 0 resamples, seed 1")
    assert motifs.stats["A"]["reported"] == 5 and motifs.stats["B"]["sample_take_part"] == 2


def test_stage_lines_follow_the_contract_and_their_order(stage):
    pipeline.main(_args(stage, "--resamples", "50", "--motif-min-count", "1", "--seed", "4"))
    for name, units in (("A", SAMPLE_A), ("B", SAMPLE_B)):
        lines = open(stage["dir"] + f"dcr_{name}.cdr3_motifs.tsv").read().split("\n")
        want = mu.expected_motifs(units, BACKGROUND, (2, 3, 4), (3, 3), 1, 50, 4)
        assert lines[0] == HEAD and lines[-1] == "" and lines[1:-1] == mu.expected_lines(want, 50)
        keys = [(int(f[5]), -int(f[2]), int(f[1]), f[0]) for f in (x.split("\t") for x in lines[1:-1])]
        assert keys == sorted(keys) and len({k[0] for k in keys}) > 1
        for f in (x.split("\t") for x in lines[1:-1]):
            assert f[4] == "50" and f[8] == format(int(f[6]) / 50, ".6f") and f[10] == format((int(f[5]) + 1) / 51, ".6f")
            assert f[9] == (format(int(f[2]) * 50 / int(f[6]), ".6f") if int(f[6]) else "nan")


def test_stage_same_seed_same_files_and_gzip(stage):
    args = [a for a in _args(stage, "--resamples", "20", "--motif-min-count", "1") if a != "-dz"]
    pipeline.main(args)
    first = gzip.open(stage["dir"] + "dcr_A.cdr3_motifs.tsv.gz", "rb").read()
    pipeline.main(args + ["-dz"])
    assert open(stage["dir"] + "dcr_A.cdr3_motifs.tsv", "rb").read() == first
    pipeline.main(args + ["-dz", "--seed", "2", "-pf", "s2_"])
    assert open(stage["dir"] + "s2_A.cdr3_motifs.tsv", "rb").read() != first


def test_stage_background_column_by_name(stage, tmp_path):
    table = tmp_path / "bg.tsv"
    table.write_bytes(b"id\tCDR3\n" + b"".join(b"%d\t%s\n" % (i, u) for i, u in enumerate(BACKGROUND)))
    pipeline.main(["motifs", "-in", stage["a"], "-bg", str(table), "--bg-cdr3-column", "CDR3", "-op", stage["dir"], "-dz", "-pf", "c_",
                   "--resamples", "5"])
    pipeline.main(_args(stage, "--resamples", "5", files=[stage["a"]]))
    assert open(stage["dir"] + "c_A.cdr3_motifs.tsv", "rb").read() == open(stage["dir"] + "dcr_A.cdr3_motifs.tsv", "rb").read()
    with pytest.raises(SystemExit):
        pipeline.main(["motifs", "-in", stage["a"], "-bg", str(table), "-op", stage["dir"], "-dz"])


def _refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        pipeline.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_stage_refusals(stage, capsys, tmp_path, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(nat, "cdr3_motifs", never)
    other = tmp_path / "x"
    other.mkdir()
    same = str(other / "A.clonotypes.tsv")
    mu.clonotype_file(same, SAMPLE_B)
    assert "two files give one sample name ('A')" in _refused(_args(stage, files=[stage["a"], same]), capsys)
    # A has 3 units that take part: a background of 2 is too small, and both numbers are named
    small = str(tmp_path / "small.clonotypes.tsv")
    mu.clonotype_file(small, BACKGROUND[:2])
    err = _refused(["motifs", "-in", stage["a"], "-bg", small, "-op", stage["dir"], "-dz"], capsys)
    assert re.search(r"\b3 CDR3s take part\b.*\bonly 2\b", err)
    for flags, words in ((["--motif-k", "2,5"], "--motif-k"), (["--motif-k", "2,2"], "--motif-k"), (["--motif-k", ""], "--motif-k"),
                         (["--motif-trim", "3"], "--motif-trim"), (["--motif-trim", "17,0"], "--motif-trim"),
                         (["--motif-trim", "0,-1"], "--motif-trim"), (["--motif-min-count", "0"], "--motif-min-count"),
                         (["--resamples", "65536"], "--resamples"), (["--resamples", "-1"], "--resamples"),
                         (["--seed", "-1"], "--seed"), (["--seed", str(1 << 64)], "--seed")):
        assert words in _refused(_args(stage, *flags), capsys), flags
    assert "1 to 64" in _refused(_args(stage, files=[stage["a"]] * 65), capsys)
    assert motifs.refusal({"infile": [stage["a"]]}).startswith("motifs takes a background")
    assert motifs.refusal({"infile": [stage["a"]], "background": "nowhere.tsv"}) is None      # decided before any file is opened


def test_r_0_runs_with_a_small_background(stage, tmp_path):
    small = str(tmp_path / "small.clonotypes.tsv")
    mu.clonotype_file(small, BACKGROUND[:2])
    out = motifs.run({"infile": [stage["a"]], "background": small, "outpath": stage["dir"], "prefix": "z_", "dontgzip": True, "resamples": 0})
    assert out["stats"][0]["background_take_part"] == 2 and os.path.exists(out["motifs"][0])


# ---- help and exports ----

def test_help_names_every_flag_and_the_other_helps_are_unchanged():
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    got = {c: subprocess.run([sys.executable, "-m", "decombinator_amd", c, "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
           for c in ("motifs", "decombine", "pipeline", "translate")}
    assert got["motifs"].returncode == 0
    for flag in ("-in", "-bg", "--bg-cdr3-column", "--motif-k", "--motif-trim", "--motif-min-count", "--resamples", "--seed", "-op", "-pf", "-dz"):
        assert flag in got["motifs"].stdout, flag
    for command in ("decombine", "pipeline", "translate"):
        with open(os.path.join(HELP_DIR, command + ".txt")) as fh:
            assert " ".join(got[command].stdout.split()) == " ".join(fh.read().split()), command
    from decombinator_amd.io import create_parser
    choices = [a.choices for a in create_parser()._actions if getattr(a, "choices", None)]
    assert [list(c) for c in choices] == [["pipeline", "decombine", "collapse", "translate", "overlap"]]
    assert "motifs" in create_parser().epilog and "match" in create_parser().epilog


def test_exports():
    names = ("dcrx_cdr3_motifs_work_bytes", "dcrx_cdr3_motifs_device", "dcrx_cdr3_motifs")
    header = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    for name in names:
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", header)
        assert hasattr(nat.lib(), name)
    assert nat.lib().dcrx_abi_version() == 5
    assert "#define DCRX_CDR3_MOTIF_MAX_RESAMPLES %d" % nat.CDR3_MOTIF_MAX_RESAMPLES in header
    assert "#define DCRX_CDR3_MOTIF_MAX_TRIM %d" % nat.CDR3_MOTIF_MAX_TRIM in header
    assert nat.cdr3_motif_k_mask((2, 3, 4)) == 0x1C and nat.cdr3_motif_k_mask([3]) == 8
    assert ctypes_size() == 8 * len(nat.CDR3_MOTIF_STATS)


def ctypes_size():
    import ctypes
    return ctypes.sizeof(nat.Cdr3MotifStatsC)
