"""`match` (include/dcrx.h "match") without a GPU: the Python contract against itself, the host walk of the kernel's steps on
the constructed lists, the host formatter, the stage's refusals and database parsing over a stubbed native call, and the
stand-alone sanitizer run of the host walk."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import match as mt
from decombinator_amd import pipeline
from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the contract in Python ----

@pytest.mark.parametrize("mode", ["none", "v", "vj"])
def test_reference_equals_all_pairs_on_random_families(mode):
    table = mu.random_case(220, 260, 3, 2, seed=11 + len(mode))
    case = mu.classed(*table, mode)
    ref = mu.Reference(case)
    for metric in mu.METRICS:
        seen = set()
        for D in (0, 1, 2):
            want = mu.expected_match_naive(case, D, metric)
            mu.assert_same(ref.expected(D, metric), want, (mode, metric, D))
            seen |= ref.distances_seen(D, metric)
            assert 0 < want["stats"]["queries_hit"] < len(case.q_strings) and 0 < want["stats"]["targets_hit"] < len(case.t_strings)
        assert seen == {0, 1, 2}
    # the indels matter: Levenshtein finds hits Hamming has not
    assert ref.expected(1, "levenshtein")["stats"]["hits"] > ref.expected(1, "hamming")["stats"]["hits"]
    # distance 0 is byte equality under either metric
    mu.assert_same(ref.expected(0, "levenshtein"), ref.expected(0, "hamming"))


def test_the_sides_are_different_sets():
    case = mu.Case([0, 0, 1], ["CASSF", "CASSF", "CASSF"], [0, 1, 2], ["CASSF", "CASSY", "CASSF"], [3, 5, 7])
    want = mu.expected_match_naive(case, 1, "hamming")
    assert want["degree"].tolist() == [2, 1, 0] and want["hit"].tolist() == [0, 1, 2]
    assert want["t_queries"].tolist() == [1, 1, 1] and want["t_weight"].tolist() == [3, 3, 5]
    assert want["stats"] == {"queries": 3, "targets": 3, "queries_out_of_reach": 0, "targets_out_of_reach": 0, "hits": 3, "queries_hit": 2,
                             "queries_hit_weight": 8, "targets_hit": 3, "largest_degree": 2}


# ---- the host walk: the kernel's steps with the shared look-ups ----

CONSTRUCTED = None


def constructed():
    global CONSTRUCTED
    if CONSTRUCTED is None:
        CONSTRUCTED = mu.constructed()
        for L in mu.EDIT_LENGTHS:
            CONSTRUCTED[f"every_edit_{L}"] = mu.every_edit(L)
    return CONSTRUCTED


def test_core_constants_and_the_range_look_up():
    h = mu.host_lib()
    assert h.cdr3match_host_queries() == 256 and h.cdr3match_host_tile() == 256
    keys = np.array(sorted([(c << 6) | n for c in (1, 1, 4, 4, 4, 9) for n in (5, 7)]) + [1 << 38] * 3, dtype=np.uint64)
    for lev in (0, 1):
        bucket = (lambda k: k >> 6) if lev else (lambda k: k)
        for k in sorted({bucket(int(x)) + d for x in keys for d in (-1, 0, 1)} | {0}):
            want = next((p for p, x in enumerate(keys) if bucket(int(x)) >= k), len(keys))
            assert h.cdr3match_host_first_at_or_above(keys.ctypes.data, len(keys), k, lev) == want, (lev, k)
        assert h.cdr3match_host_first_at_or_above(keys.ctypes.data, 0, 5, lev) == 0


@pytest.mark.parametrize("metric", mu.METRICS)
def test_host_walk_gives_the_contract_on_the_constructed_lists(metric):
    blocks = set()
    for name, case in constructed().items():
        for side in (case, case.swapped()):
            blocks.add((len(side.q_strings) + 255) // 256)
            for D in (0, 1, 2):
                want = mu.expected_match_naive(side, D, metric)
                degree, hit_off, hit = mu.host_match(side, D, metric)
                assert np.array_equal(degree, want["degree"]), (name, D)
                assert np.array_equal(hit_off, want["hit_off"]) and np.array_equal(hit, want["hit"]), (name, D)
    assert {1, 2, 3} <= blocks and max(blocks) >= 6      # query grids of one block, three, and many


def test_host_walk_on_random_families():
    case = mu.classed(*mu.random_case(400, 600, 5, 2, seed=2), "v")
    for metric in mu.METRICS:
        for D in (0, 1, 2):
            want = mu.expected_match_naive(case, D, metric)
            degree, hit_off, hit = mu.host_match(case, D, metric)
            assert np.array_equal(degree, want["degree"]) and np.array_equal(hit, want["hit"]) and want["stats"]["hits"] > 0


def test_sanitizer_run_of_the_host_walk():
    """The stand-alone program (its own main) under AddressSanitizer and UBSan: host code, on the CPU."""
    got = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_cdr3match"), "asan"], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-2000:]
    assert got.stdout.strip().endswith("ok") and "rows differ" in got.stdout


# ---- the host formatter ----

def test_format_cdr3_matches_against_python():
    ts, tv, tj, qs, qv, qj = mu.random_case(120, 150, 3, 2, seed=5)
    ts[3], qs[4] = "CA\x80\xffSS", "CA\x80\xffSS"          # bytes >= 0x80 are written as they are
    case = mu.classed(ts, tv, tj, qs, qv, qj, "v")
    db_header = [b"cdr3", b"v", b"epitope"]
    db_lines = [b"\t".join([t, v.encode(), b"EPI%d" % k]) for k, (t, v) in enumerate(zip(case.t_strings, tv))]
    q_off, q_text = cnu.node_text(case.q_strings)
    t_off, t_text = cnu.node_text(case.t_strings)
    v_calls, j_calls = sorted(set(qv)), sorted(set(qj))
    for metric in mu.METRICS:
        for D in (0, 2):
            result = mu.expected_match_naive(case, D, metric)
            assert result["stats"]["hits"] > 0
            got = nat.format_cdr3_matches(result, [v_calls.index(x) for x in qv], [j_calls.index(x) for x in qj], v_calls, j_calls, q_off,
                                          q_text, case.weights, t_off, t_text, b"\t".join(b"db_" + h for h in db_header), db_lines, metric)
            assert got == mu.matches_text(qv, qj, case, result, db_header, db_lines, metric), (metric, D)
    none = mu.expected_match_naive(mu.Case(case.t_classes, case.t_strings, [], []), 1, "hamming")
    assert nat.format_cdr3_matches(none, [], [], [], [], np.zeros(1, np.uint64), b"", [], t_off, t_text, b"db_x", db_lines) == \
        b"\t".join(c.encode() for c in nat.CDR3_MATCH_COLUMNS) + b"\tdb_x\n"


def test_format_cdr3_matches_refuses_what_does_not_fit():
    case = mu.Case([0, 0], ["CASS", "CASSF"], [0], ["CASS"], [1])
    result = mu.expected_match_naive(case, 1, "levenshtein")
    assert result["hit"].tolist() == [0, 1]
    q_off, q_text = cnu.node_text(case.q_strings)
    t_off, t_text = cnu.node_text(case.t_strings)
    args = ([0], [0], ["V"], ["J"], q_off, q_text, [1], t_off, t_text, b"db_a", [b"x", b"y"])
    assert nat.format_cdr3_matches(result, *args, "levenshtein").splitlines()[2] == b"0\tV\tJ\tCASS\t1\t1\t1\ty"
    with pytest.raises(nat.DcrxError, match="two lengths"):
        nat.format_cdr3_matches(result, *args, "hamming")
    with pytest.raises(nat.DcrxError, match="outside the targets"):
        nat.format_cdr3_matches(dict(result, hit=np.array([0, 2], np.uint32)), *args, "levenshtein")


# ---- the stage over a stubbed native call ----

A_ROWS = [("TRBV1*01", "TRBJ1*01", "CASSF", 10), ("TRBV1*02", "TRBJ1*01", "CASSY", 5), ("TRBV2*01", "TRBJ2*01", "CASSF", 1),
          ("TRBV1*01", "TRBJ1*01", "CASSLF", 2)]
B_ROWS = [("TRBV1*01", "TRBJ2*01", "CASSW", 20), ("TRBV3*01", "TRBJ1*01", "CAWWW", 4)]
DB = (b"CDR3\tV\tJ\tEpitope\n"
      b"CASSF\tTRBV1*01\tTRBJ1*01\tGIL\n"
      b"CASSY\tTRBV1*01\tTRBJ1*01\tNLV\n"
      b"CASSF\tTRBV2*01\tTRBJ2*01\tGLC\n"
      b"CAWWWW\tTRBV3*01\tTRBJ1*01\tELA\n")
DB_FLAGS = dict(db_cdr3_column="CDR3", db_v_column="V", db_j_column="J")


def clonotypes_text(rows) -> bytes:
    lines = ["\t".join(nat.CLONOTYPE_COLUMNS)]
    for v, j, aa, dup in rows:
        lines.append("\t".join([v, j, aa, str(dup)] + ["0"] * (len(nat.CLONOTYPE_COLUMNS) - 4)))
    return ("\n".join(lines) + "\n").encode()


def write_inputs(tmp_path, tables, db=DB, db_name="known.tsv"):
    files = []
    for name, rows in tables:
        path = str(tmp_path / (name + ".clonotypes.tsv"))
        with open(path, "wb") as fh:
            fh.write(clonotypes_text(rows))
        files.append(path)
    db_path = str(tmp_path / db_name)
    with (gzip.open if db_name.endswith(".gz") else open)(db_path, "wb") as fh:
        fh.write(db)
    return files, db_path


def stage(tmp_path, monkeypatch, files, db_path, calls=None, **kw):
    mu.StubIndex.made.clear()
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_match", mu.brute_force_native(calls))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out, exist_ok=True)
    inp = dict(command="match", infile=files, database=db_path, outpath=out, prefix="t_", dontgzip=True, cdr3_distance=1,
               cdr3_metric="hamming", cdr3_class="v", strip_alleles=False, db_cdr3_column="junction_aa", db_v_column="v_call",
               db_j_column="j_call")
    inp.update(kw)
    res = mt.run(inp)
    read = lambda p: (gzip.open if p.endswith(".gz") else open)(p, "rb").read()
    return [read(p) for p in res["matches"]], read(res["targets"]), res


def test_hand_case_byte_for_byte(tmp_path, monkeypatch, capsys):
    files, db = write_inputs(tmp_path, [("A", A_ROWS), ("B", B_ROWS)])
    calls = []
    matches, targets, res = stage(tmp_path, monkeypatch, files, db, calls, **DB_FLAGS)
    head = b"clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\ttarget\tdistance\tdb_CDR3\tdb_V\tdb_J\tdb_Epitope\n"
    assert matches[0] == head + (b"0\tTRBV1*01\tTRBJ1*01\tCASSF\t10\t0\t0\tCASSF\tTRBV1*01\tTRBJ1*01\tGIL\n"
                                 b"0\tTRBV1*01\tTRBJ1*01\tCASSF\t10\t1\t1\tCASSY\tTRBV1*01\tTRBJ1*01\tNLV\n"
                                 b"2\tTRBV2*01\tTRBJ2*01\tCASSF\t1\t2\t0\tCASSF\tTRBV2*01\tTRBJ2*01\tGLC\n")
    assert matches[1] == head + (b"0\tTRBV1*01\tTRBJ2*01\tCASSW\t20\t0\t1\tCASSF\tTRBV1*01\tTRBJ1*01\tGIL\n"
                                 b"0\tTRBV1*01\tTRBJ2*01\tCASSW\t20\t1\t1\tCASSY\tTRBV1*01\tTRBJ1*01\tNLV\n")
    assert targets == (b"target\tdb_CDR3\tdb_V\tdb_J\tdb_Epitope\tA_clonotypes\tA_reads\tB_clonotypes\tB_reads\n"
                       b"0\tCASSF\tTRBV1*01\tTRBJ1*01\tGIL\t1\t10\t1\t20\n"
                       b"1\tCASSY\tTRBV1*01\tTRBJ1*01\tNLV\t1\t10\t1\t20\n"
                       b"2\tCASSF\tTRBV2*01\tTRBJ2*01\tGLC\t1\t1\t0\t0\n")
    assert [os.path.basename(p) for p in res["matches"]] == ["t_A.cdr3_matches.tsv", "t_B.cdr3_matches.tsv"]
    assert os.path.basename(res["targets"]) == "t_match_targets.tsv" and oct(os.stat(res["targets"]).st_mode)[-3:] == "666"
    # ONE index, and every sample ONE call against it; classes numbered from the V strings over the database and all samples
    assert len(mu.StubIndex.made) == 1 and mu.StubIndex.made[0].closed and len(calls) == 2 and calls[0][0] is calls[1][0]
    assert mu.StubIndex.made[0].classes == [0, 0, 1, 2] and calls[0][1] == [0, 3, 1, 0] and calls[1][1] == [0, 2]
    assert calls[0][4:] == (1, "hamming") and calls[0][3] == [10, 5, 1, 2]
    printed = capsys.readouterr().out.splitlines()
    assert printed[0] == ("Match of A against 4 database entries (hamming 1, class v): 4 clonotypes, 2 with a hit (11 reads), 3 hits, "
                          "0 clonotypes and 0 entries out of reach")
    assert mt.stats["B"]["hits"] == 2


def test_strip_alleles_class_modes_metric_and_gz(tmp_path, monkeypatch):
    files, db = write_inputs(tmp_path, [("A", A_ROWS), ("B", B_ROWS)], db_name="known.tsv.gz")
    calls = []
    matches, targets, res = stage(tmp_path, monkeypatch, files, db, calls, strip_alleles=True, dontgzip=False, **DB_FLAGS)
    assert res["targets"].endswith("match_targets.tsv.gz") and res["matches"][0].endswith("A.cdr3_matches.tsv.gz")
    assert calls[0][1] == [0, 0, 1, 0]                       # TRBV1*02 is TRBV1 now: CASSY of sample A hits
    assert b"1\tTRBV1*02\tTRBJ1*01\tCASSY\t5\t1\t0\tCASSY" in matches[0]
    # class vj: the J call is read too; CASSW of B (TRBJ2) no longer shares a class with the TRBV1 / TRBJ1 entries
    matches, _, _ = stage(tmp_path, monkeypatch, files, db, cdr3_class="vj", **DB_FLAGS)
    assert len(matches[1].splitlines()) == 1
    # class none and Levenshtein 1: CASSLF of A is one residue from CASSF (both entries), CAWWW of B from CAWWWW
    calls = []
    matches, targets, _ = stage(tmp_path, monkeypatch, files, db, calls, cdr3_class="none", cdr3_metric="levenshtein", **DB_FLAGS)
    assert set(calls[0][1]) == {0} and calls[0][5] == "levenshtein"
    assert [ln.split(b"\t")[5:7] for ln in matches[0].splitlines() if ln.startswith(b"3\t")] == [[b"0", b"1"], [b"2", b"1"]]
    assert matches[1].splitlines()[-1].split(b"\t")[3:8] == [b"CAWWW", b"4", b"3", b"1", b"CAWWWW"]
    assert targets.splitlines()[-1].startswith(b"3\tCAWWWW\tTRBV3*01\tTRBJ1*01\tELA\t0\t0\t1\t4")


def test_a_clonotype_table_is_a_database_as_it_stands(tmp_path, monkeypatch):
    files, _ = write_inputs(tmp_path, [("A", A_ROWS), ("B", B_ROWS)])
    matches, targets, res = stage(tmp_path, monkeypatch, files[:1], files[1], cdr3_distance=1)
    lines = matches[0].splitlines()
    assert lines[0].split(b"\t")[7:11] == [b"db_v_call", b"db_j_call", b"db_junction_aa", b"db_duplicate_count"]
    assert [ln.split(b"\t")[:7] for ln in lines[1:]] == [[b"0", b"TRBV1*01", b"TRBJ1*01", b"CASSF", b"10", b"0", b"1"]]
    assert lines[1].split(b"\t")[7:11] == [b"TRBV1*01", b"TRBJ2*01", b"CASSW", b"20"]


def _no_open(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a file was opened, or the device called, before the refusal")
    monkeypatch.setattr(mt, "read_table", boom)
    monkeypatch.setattr(mt, "read_database", boom)
    monkeypatch.setattr(nat, "Cdr3Index", boom)
    monkeypatch.setattr(nat, "cdr3_match", boom)


@pytest.mark.parametrize("files,kw,msg", [
    ([], {}, "1 to 64"),
    ([f"s{k}.clonotypes.tsv" for k in range(65)], {}, "1 to 64"),
    (["x/a.clonotypes.tsv", "y/a.clonotypes.tsv.gz"], {}, "one sample name"),
    (["a.clonotypes.tsv"], {"cdr3_distance": 3}, "--cdr3-distance"),
    (["a.clonotypes.tsv"], {"cdr3_distance": -1}, "--cdr3-distance"),
])
def test_refusals_before_anything_is_opened(monkeypatch, files, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="match", infile=files, database="db.tsv", outpath="", prefix="", dontgzip=True)
    inp.update(kw)
    assert msg in mt.refusal(inp)
    with pytest.raises(ValueError, match=msg):
        mt.run(inp)


def test_refusal_from_the_command_line(monkeypatch, capsys):
    _no_open(monkeypatch)
    with pytest.raises(SystemExit) as e:
        pipeline.main(["match", "-in", "a.clonotypes.tsv", "-db", "db.tsv", "--cdr3-distance", "3"])
    assert e.value.code == 2 and "--cdr3-distance" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pipeline.main(["match", "-in", "a.clonotypes.tsv"])      # no database


def test_database_refusals_come_before_any_device_call(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was called before the refusal")
    files, db = write_inputs(tmp_path, [("A", A_ROWS)])
    run = lambda **kw: mt.run(dict(command="match", infile=files, database=db, outpath=str(tmp_path) + os.sep, prefix="", dontgzip=True, **kw))
    monkeypatch.setattr(nat, "Cdr3Index", boom)
    monkeypatch.setattr(nat, "cdr3_match", boom)
    with pytest.raises(ValueError, match="no column 'junction_aa'"):
        run()
    with pytest.raises(ValueError, match=r"no column 'v_call' \(--db-v-column\)"):
        run(db_cdr3_column="CDR3")
    with pytest.raises(ValueError, match="no column 'j_call'"):
        run(db_cdr3_column="CDR3", db_v_column="V", cdr3_class="vj")
    files, db = write_inputs(tmp_path, [("A", A_ROWS)], db=DB + b"CASSQ\tTRBV1*01\n")
    with pytest.raises(ValueError, match="line 6: 2 fields"):
        run(**DB_FLAGS)
    # class none needs the CDR3 column alone: the database may lack the calls
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_match", mu.brute_force_native())
    files, db = write_inputs(tmp_path, [("A", A_ROWS)], db=b"name\tCDR3\nx\tCASSY\n")
    res = run(db_cdr3_column="CDR3", cdr3_class="none")
    assert res["stats"][0]["hits"] == 3


def test_duplicate_counts_that_add_up_to_2_64_are_refused_by_the_files_name(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the sample went to the device before the refusal")
    rows = [("TRBV1*01", "TRBJ1*01", "CASSF", (1 << 63)), ("TRBV1*01", "TRBJ1*01", "CASSY", (1 << 63))]
    files, db = write_inputs(tmp_path, [("A", rows)])
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_match", boom)
    inp = dict(command="match", infile=files, database=db, outpath=str(tmp_path) + os.sep, prefix="", dontgzip=True, **DB_FLAGS)
    with pytest.raises(ValueError, match=r"A\.clonotypes\.tsv: the duplicate counts add up to 2\^64 or more"):
        mt.run(inp)
    assert mu.StubIndex.made[-1].closed
    # one count of 2^64 alone (no uint64 holds it), and from the command line: the parser's error, not a traceback
    files, db = write_inputs(tmp_path, [("A", [("TRBV1*01", "TRBJ1*01", "CASSF", 1 << 64)])])
    with pytest.raises(SystemExit) as e:
        pipeline.main(["match", "-in", *files, "-db", db, "-op", str(tmp_path) + os.sep, "--db-cdr3-column", "CDR3", "--db-v-column", "V",
                       "--db-j-column", "J"])
    assert e.value.code == 2
    # one below is accepted
    rows[1] = rows[1][:3] + ((1 << 63) - 1,)
    files, db = write_inputs(tmp_path, [("A", rows)])
    monkeypatch.setattr(nat, "cdr3_match", mu.brute_force_native())
    assert mt.run(inp)["stats"][0]["queries_hit_weight"] == (1 << 64) - 1


def test_the_parser_of_match():
    from decombinator_amd.io import cli_args
    inp = cli_args(["match", "-in", "a.clonotypes.tsv", "b.clonotypes.tsv", "-db", "k.tsv"])
    assert inp["command"] == "match" and inp["infile"] == ["a.clonotypes.tsv", "b.clonotypes.tsv"] and inp["database"] == "k.tsv"
    assert (inp["cdr3_distance"], inp["cdr3_metric"], inp["cdr3_class"], inp["strip_alleles"]) == (1, "hamming", "v", False)
    assert (inp["db_cdr3_column"], inp["db_v_column"], inp["db_j_column"]) == ("junction_aa", "v_call", "j_call")
    assert inp["prefix"] == "dcr_" and inp["outpath"] == "" and inp["dontgzip"] is False
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    import sys
    got = subprocess.run([sys.executable, "-m", "decombinator_amd", "match", "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert got.returncode == 0 and all(f in got.stdout for f in ("--cdr3-distance", "--strip-alleles", "--db-cdr3-column", "-db"))


def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr
    for name in ("dcrx_cdr3_index_create", "dcrx_cdr3_index_info", "dcrx_cdr3_index_destroy", "dcrx_cdr3_match_work_bytes",
                 "dcrx_cdr3_match_device", "dcrx_cdr3_match_run", "dcrx_cdr3_match_info", "dcrx_cdr3_match_export",
                 "dcrx_cdr3_match_destroy", "dcrx_format_cdr3_matches"):
        assert name in nat.EXPORTS and name + "(" in hdr and hasattr(nat.lib(), name)
    assert nat.cdr3_match_work_bytes(1 << 30, 0) == 0 and nat.cdr3_match_work_bytes(10, 0, 7) == 0
