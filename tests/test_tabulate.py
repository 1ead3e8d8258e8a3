"""The tally (include/dcrx.h "tally, weighted") and the `tabulate` sub-command without a GPU: the host walk with the per-entry
bound and the tally sink (tests/host_cdr3tally) against the contract (tests/cdr3_tally_util.py) on every constructed list of
tests/cdr3_wmatch_util.py under three patterns of radii, the stand-alone program, the exports, the refusals the entries decide on
the host before any device call, and the stage with the native calls replaced by the contract against files written by hand,
its refusals and its help."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from decombinator_amd import tabulate as tb
from tests import cdr3_match_util as mu
from tests import cdr3_tally_util as tu
from tests import cdr3_wmatch_util as wu
from tests.test_cdr3_match import clonotypes_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2


# ---- the contract's two forms agree ----

@pytest.mark.parametrize("name", ["targets_257", "queries_513", "non_letters", "gap_d4_inside", "sums_past_2_12"])
def test_the_numpy_form_is_the_brute_force(name):
    case, cost, R = wu.constructed()[name]
    for pattern in tu.PATTERNS:
        radii = tu.radii_for(pattern, R, len(case.t_strings))
        tu.assert_same(tu.expected_tally_numpy(case, cost, radii), tu.expected_tally(case, cost, radii), (name, pattern))


def test_with_one_radius_the_contract_is_the_weighted_match():
    case, cost, R = wu.constructed()["targets_257"]
    want, got = wu.expected(case, cost, R), tu.expected_tally(case, cost, tu.radii_for("all_R", R, len(case.t_strings)))
    assert np.array_equal(got["t_count"], want["t_queries"]) and np.array_equal(got["t_weight"], want["t_weight"])
    assert np.array_equal(got["q_degree"], want["degree"]) and got["stats"]["hits"] == want["stats"]["hits"] > 0
    graded = tu.expected_tally(case, cost, tu.radii_for("graded", R, len(case.t_strings)))
    assert 0 < graded["stats"]["hits"] < got["stats"]["hits"]      # the premise: the patterns differ
    none = tu.expected_tally(case, cost, tu.radii_for("every_third_none", R, len(case.t_strings)))
    assert not none["t_count"][2::3].any() and none["stats"]["targets_without_radius"] == len(case.t_strings) // 3


# ---- the host walk with WeightedPer and the tally sink ----

@pytest.mark.parametrize("name", wu.NAMES)
def test_host_walk_against_the_contract(name):
    case, cost, R = wu.constructed()[name]
    blocks = -(-len(case.q_strings) // 256)
    for pattern in tu.PATTERNS:
        radii = tu.radii_for(pattern, R, len(case.t_strings))
        want = tu.expected_tally(case, cost, radii)
        got = tu.host_tally(case, cost, radii)
        tu.assert_same({k: got[k] for k in ("t_count", "t_weight", "q_degree")}, want, (name, pattern))
        assert got["flushes"] <= want["stats"]["targets_hit"] * blocks      # at most one flush per (block, target that is hit)


def test_host_walk_treats_a_value_above_65535_as_no_radius():
    case, cost, R = wu.constructed()["targets_257"]
    radii = tu.radii_for("all_R", R, len(case.t_strings))
    radii[::2] = 65536
    radii[1] = 0xFFFFFFFE
    got, want = tu.host_tally(case, cost, radii), tu.expected_tally(case, cost, radii)
    tu.assert_same({k: got[k] for k in ("t_count", "t_weight", "q_degree")}, want)
    assert not got["t_count"][::2].any() and got["t_count"][1] == 0 and got["t_count"].any()


def test_the_stand_alone_program_plain():
    """The walk, the three patterns of radii and the refused radii in a program of its own (its own main; `make asan` builds the
    same source under AddressSanitizer and UBSan), never loaded into Python."""
    tu.host_lib()
    plain = subprocess.run([os.path.join(tu.HOST_DIR, "build", "cdr3tally_main")], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "ok", plain.stdout[-2000:]
    assert "a class between two" in plain.stdout and "the radii the host entry refuses: 0 differ" in plain.stdout


# ---- exports and ABI ----

def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    for name in ("dcrx_cdr3_tally_weighted_work_bytes", "dcrx_cdr3_tally_weighted_device", "dcrx_cdr3_tally_weighted"):
        assert name in nat.EXPORTS and re.search(r"\b" + name + r"\(", hdr) and hasattr(nat.lib(), name)
    assert "tally, weighted" in hdr and "#define DCRX_CDR3_NO_RADIUS 0xFFFFFFFFu" in hdr and nat.CDR3_NO_RADIUS == 0xFFFFFFFF == tu.NO_RADIUS
    assert "treated on the device as DCRX_CDR3_NO_RADIUS" in " ".join(hdr.split())
    fields = re.search(r"typedef struct dcrx_cdr3_tally_stats \{(.*?)\}", hdr, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == nat.CDR3_TALLY_STATS
    assert C.sizeof(nat.Cdr3TallyStatsC) == 8 * len(nat.CDR3_TALLY_STATS)
    assert callable(nat.cdr3_tally_weighted) and callable(nat.cdr3_tally_weighted_device)


def test_work_bytes_are_answered_on_the_host():
    need = nat.cdr3_tally_weighted_work_bytes(1000, 0, 500)
    assert need % 256 == 0 and need >= nat.cdr3_profile_weighted_work_bytes(1000, 0, 1) + 500 * 12
    more = nat.cdr3_tally_weighted_work_bytes(1000, 0, 100000) - need      # linear in the targets: 12 bytes each, in two 256-byte slots
    assert abs(more - 99500 * 12) <= 512
    assert nat.cdr3_tally_weighted_work_bytes(1000, 12345, 500) == need
    assert nat.cdr3_tally_weighted_work_bytes(0, 0, 0) > 0 and nat.cdr3_tally_weighted_work_bytes(1, 5, 1) > 0
    assert nat.cdr3_tally_weighted_work_bytes(1 << 30, 0, 1) == 0 and nat.cdr3_tally_weighted_work_bytes(1, 0, 1 << 30) == 0


# ---- the refusals of both entries: on the host, before any device call (an index of no targets touches no device) ----

def _empty_index():
    return nat.Cdr3Index(np.zeros(0, np.uint32), np.zeros(1, np.uint64), b"")


def _bad_costs():
    ok = nat.Cdr3Cost.default()
    asym, diag = ok.sub.copy(), ok.sub.copy()
    asym[1, 3] = 5
    diag[26, 26] = 1
    return [(nat.Cdr3Cost(asym), "symmetric"), (nat.Cdr3Cost(diag), "diagonal"), (nat.Cdr3Cost.default(gap=0), "gap"),
            (nat.Cdr3Cost.default(gap=256), "gap"), (nat.Cdr3Cost.default(ntrim=17), "trim"), (nat.Cdr3Cost.default(ctrim=17), "trim"),
            (None, "null cost")]


class _Fake:
    """Something with a .ptr: an address the entry must refuse before it looks behind it."""

    def __init__(self, ptr):
        self.ptr = ptr


def test_both_entries_refuse_what_the_contract_refuses():
    index = _empty_index()
    cls, off, text, w, none = np.zeros(1, np.uint32), np.array([0, 5], np.uint64), b"CASSF", np.ones(1, np.uint64), np.zeros(0, np.uint32)
    try:
        for cost, msg in _bad_costs():
            with pytest.raises(nat.DcrxError, match=msg) as e:
                nat.cdr3_tally_weighted(index, cls, off, text, w, cost, none)
            assert e.value.code == E_INVALID
            with pytest.raises(nat.DcrxError, match=msg) as e:
                nat.cdr3_tally_weighted_device(index, 0, None, None, None, 0, None, cost, None, None, None, None, None, 0)
            assert e.value.code == E_INVALID
        ok, L = nat.Cdr3Cost.default(), nat.lib()
        c = ok.as_c()
        t = np.frombuffer(b"CASSF\0", np.uint8)
        deg = np.full(1, 0xA5A5A5A5, np.uint32)
        call = lambda i, m, o, wt, d: L.dcrx_cdr3_tally_weighted(i, m, cls.ctypes.data, o.ctypes.data, t.ctypes.data, wt.ctypes.data, C.addressof(c),
                                                                 None, None, None, d, None)
        # a null output with a non-zero size, on both entries; a null index; offsets that go backwards; a weight sum of 2^64
        assert call(index.handle, 1, off, w, None) == E_INVALID and b"null output" in L.dcrx_last_error()
        with pytest.raises(nat.DcrxError, match="null output"):
            nat.cdr3_tally_weighted_device(index, 1, _Fake(256), _Fake(256), _Fake(256), 5, _Fake(256), ok, None, None, None, None, _Fake(256), 1 << 20)
        assert call(None, 1, off, w, deg.ctypes.data) == E_INVALID
        assert L.dcrx_cdr3_tally_weighted_device(None, 0, None, None, None, 0, None, C.addressof(c), None, None, None, None, None, 0, None) == E_INVALID
        back = np.array([5, 0], np.uint64)
        assert call(index.handle, 1, back, w, deg.ctypes.data) == E_INVALID and b"backwards" in L.dcrx_last_error()
        cls2, off2, w2, deg2 = np.zeros(2, np.uint32), np.array([0, 2, 5], np.uint64), np.array([1 << 63, 1 << 63], np.uint64), np.zeros(2, np.uint32)
        assert L.dcrx_cdr3_tally_weighted(index.handle, 2, cls2.ctypes.data, off2.ctypes.data, t.ctypes.data, w2.ctypes.data, C.addressof(c), None,
                                          None, None, deg2.ctypes.data, None) == E_UNSUPPORTED and b"2^64" in L.dcrx_last_error()
        assert deg[0] == 0xA5A5A5A5      # (no refusal wrote anything)
        assert L.dcrx_cdr3_tally_weighted_device(index.handle, 1 << 30, None, None, None, 0, None, C.addressof(c), None, None, None, None, None, 0,
                                                 None) == E_UNSUPPORTED
        # the binding: one radius per target, each of 32 bits
        with pytest.raises(ValueError, match="radii for 0 targets"):
            nat.cdr3_tally_weighted(index, cls, off, text, w, ok, [3])
        with pytest.raises(ValueError, match="32 bits"):
            nat.cdr3_tally_weighted(index, cls, off, text, w, ok, [-1])
    finally:
        index.close()


def test_the_radii_the_host_entry_refuses():
    """refuse_radii of the shared header, which the host entry asks before any device call: 65536 .. 0xFFFFFFFE."""
    assert not tu.host_refuses([]) and not tu.host_refuses([0, 1, 65535, tu.NO_RADIUS])
    for bad in (65536, 70000, 1 << 31, 0xFFFFFFFE):
        assert tu.host_refuses([0, bad]) and tu.host_refuses([bad, tu.NO_RADIUS]), bad


def test_no_queries_and_no_targets_are_answered_on_the_host():
    index = _empty_index()
    try:
        ok, none = nat.Cdr3Cost.default(), np.zeros(0, np.uint32)
        got = nat.cdr3_tally_weighted(index, none, np.zeros(1, np.uint64), b"", np.zeros(0, np.uint64), ok, none)
        assert [len(got[k]) for k in ("t_count", "t_weight", "q_degree")] == [0, 0, 0] and got["stats"] == dict.fromkeys(nat.CDR3_TALLY_STATS, 0)
        nat.cdr3_tally_weighted_device(index, 0, None, None, None, 0, None, ok, None, None, None, None, None, 0)      # nothing to write: no device call
        strings = [b"CASSF", b"", b"CAS*F", b"A" * 33, b"CASSW"]
        off = np.zeros(6, np.uint64)
        off[1:] = np.cumsum([len(s) for s in strings])
        got = nat.cdr3_tally_weighted(index, np.zeros(5, np.uint32), off, b"".join(strings), np.arange(1, 6, dtype=np.uint64), ok, none)
        assert got["q_degree"].tolist() == [0] * 5      # (the buffer came uncleared: every cell was written)
        assert got["stats"] == {"queries": 5, "targets": 0, "queries_out_of_reach": 2, "queries_not_letters": 1, "targets_out_of_reach": 0,
                                "targets_without_radius": 0, "hits": 0, "queries_hit": 0, "queries_hit_weight": 0, "targets_hit": 0}
    finally:
        index.close()


# ---- the stage, with the contract in the native call's place ----

MC_HEAD = b"clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\tradius\tbackground_neighbours\tbackground\tsample_neighbours\n"
MC = MC_HEAD + (
    b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t3\t0\t4\t1\n"         # 0: radius 3 ...
    b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t5\t12\t1\t4\t2\n"         # 1: ... and radius 12, I-V 3 apart: they share clonotypes
    b"2\tTRBV1*01\tTRBJ1*01\tCASSWRSSYEQYF\t5\t.\t.\t4\t.\n"          # 2: no radius: left out
    b"3\tTRBV1*01\tTRBJ1*01\tCASS*RSSYEQYF\t5\t12\t0\t4\t0\n"         # 3: a non-letter: takes no part, keeps its line
    b"4\tTRBV2*01\tTRBJ1*01\tCASSDRSSYEQYF\t5\t6\t0\t4\t0\n")         # 4: matched by nothing (the one TRBV2 clonotype is 12 away)
S1 = [("TRBV1*01", "TRBJ1*01", "CASSIRSSYEQYF", 10),      # inside 0 (at 0) and 1 (at 3)
      ("TRBV1*01", "TRBJ1*01", "CASSVRSSYEQYF", 5),       # inside 0 (at 3: exactly its radius) and 1 (at 0)
      ("TRBV1*01", "TRBJ1*01", "CASSLRSSYEQYF", 3),       # 6 from 0: outside; 9 from 1: inside
      ("TRBV1*01", "TRBJ1*01", "CASSIRSS*EQYF", 2),       # takes no part
      ("TRBV2*01", "TRBJ1*01", "CASSIRSSYEQYF", 1)]       # its class holds 4 alone, 12 away
S2 = [("TRBV1*01", "TRBJ1*01", "CASSWRSSYEQYF", 4),       # 12 from 0: outside; 12 from 1: exactly its radius
      ("TRBV3*01", "TRBJ1*01", "CASSIRSSYEQYF", 6)]       # a class no meta-clonotype has


def write_inputs(tmp_path, tables, mc=MC, mc_name="A.cdr3_metaclonotypes.tsv"):
    files = []
    for name, rows in tables:
        path = str(tmp_path / (name + ".clonotypes.tsv"))
        with open(path, "wb") as fh:
            fh.write(clonotypes_text(rows))
        files.append(path)
    mc_path = str(tmp_path / mc_name)
    with open(mc_path, "wb") as fh:
        fh.write(mc)
    return files, mc_path


def stage(tmp_path, monkeypatch, files, mc_path, calls=None, **kw):
    mu.StubIndex.made.clear()
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_tally_weighted", tu.brute_force_native(calls))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out, exist_ok=True)
    inp = dict(command="tabulate", infile=files, metaclonotypes=mc_path, outpath=out, prefix="t_", dontgzip=True)
    inp.update(kw)
    return tb.run(inp), out


def test_the_two_files_byte_for_byte(tmp_path, monkeypatch, capsys):
    cost = wu.default_cost()
    d = lambda a, b: wu.dist(a.encode(), b.encode(), cost)
    assert (d("CASSIRSSYEQYF", "CASSVRSSYEQYF"), d("CASSIRSSYEQYF", "CASSLRSSYEQYF"), d("CASSVRSSYEQYF", "CASSLRSSYEQYF")) == (3, 6, 9)
    assert (d("CASSIRSSYEQYF", "CASSWRSSYEQYF"), d("CASSVRSSYEQYF", "CASSWRSSYEQYF"), d("CASSDRSSYEQYF", "CASSIRSSYEQYF")) == (12, 12, 12)
    files, mc = write_inputs(tmp_path, [("S1", S1), ("S2", S2)])
    calls = []
    res, out = stage(tmp_path, monkeypatch, files, mc, calls)
    assert res["tabulate"] == out + "t_tabulate.tsv" and res["samples"] == out + "t_tabulate_samples.tsv"
    assert open(res["tabulate"], "rb").read() == (
        b"metaclonotype\tv_call\tj_call\tjunction_aa\tradius\tsamples\tS1_clonotypes\tS1_reads\tS2_clonotypes\tS2_reads\n"
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t3\t1\t2\t15\t0\t0\n"
        b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t12\t2\t3\t18\t1\t4\n"
        b"3\tTRBV1*01\tTRBJ1*01\tCASS*RSSYEQYF\t12\t0\t0\t0\t0\t0\n"
        b"4\tTRBV2*01\tTRBJ1*01\tCASSDRSSYEQYF\t6\t0\t0\t0\t0\t0\n")
    assert open(res["samples"], "rb").read() == (
        b"sample\tclonotypes\treads\ttake_part\tclonotypes_inside\treads_inside\tmetaclonotypes_found\n"
        b"S1\t5\t21\t4\t3\t18\t2\n"
        b"S2\t2\t10\t2\t1\t4\t1\n")
    # ONE index over the four rows with a radius, one call per sample against it, classes numbered over -mc and all samples
    assert len(mu.StubIndex.made) == 1 and mu.StubIndex.made[0].classes == [0, 0, 0, 1] and len(calls) == 2
    assert all(c[0] is mu.StubIndex.made[0] and c[5] == [3, 12, 12, 6] for c in calls)
    assert calls[0][1] == [0, 0, 0, 0, 1] and calls[1][1] == [0, 2] and calls[0][3] == [10, 5, 3, 2, 1]
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Tabulated ")]
    assert len(lines) == 2 and lines[0].startswith("Tabulated S1 against 4 meta-clonotypes (1 more left out without a radius, 1 centroids take no part")
    assert "3 clonotypes with 18 reads inside a meta-clonotype, 2 meta-clonotypes found" in lines[0]
    assert tb.stats["S2"] == {"clonotypes": 2, "reads": 10, "take_part": 2, "clonotypes_inside": 1, "reads_inside": 4, "metaclonotypes_found": 1}


def test_other_columns_classes_and_gzip(tmp_path, monkeypatch):
    import gzip
    mc = (b"id\tcdr3\tV\tr\n" b"a\tCASSIRSSYEQYF\tTRBV1*02\t3\n" b"b\tCASSVRSSYEQYF\tTRBV9*01\t12\n")
    files, path = write_inputs(tmp_path, [("S1", S1)], mc, "mine.tsv")
    flags = dict(mc_cdr3_column="cdr3", mc_v_column="V", mc_radius_column="r")
    res, _ = stage(tmp_path, monkeypatch, files, path, **flags)      # class v, alleles kept: TRBV1*02 is nobody's class
    assert open(res["tabulate"], "rb").read().splitlines()[1:] == [b"0\tTRBV1*02\t\tCASSIRSSYEQYF\t3\t0\t0\t0", b"1\tTRBV9*01\t\tCASSVRSSYEQYF\t12\t0\t0\t0"]
    res, _ = stage(tmp_path, monkeypatch, files, path, strip_alleles=True, **flags)
    assert open(res["tabulate"], "rb").read().splitlines()[1:] == [b"0\tTRBV1*02\t\tCASSIRSSYEQYF\t3\t1\t2\t15", b"1\tTRBV9*01\t\tCASSVRSSYEQYF\t12\t0\t0\t0"]
    res, _ = stage(tmp_path, monkeypatch, files, path, cdr3_class="none", dontgzip=False, **dict(flags, mc_v_column="nope"))      # (not needed: not read)
    assert res["tabulate"].endswith("t_tabulate.tsv.gz")
    assert gzip.open(res["tabulate"], "rb").read().splitlines()[1:] == [b"0\t\t\tCASSIRSSYEQYF\t3\t1\t3\t16", b"1\t\t\tCASSVRSSYEQYF\t12\t1\t4\t19"]


# ---- refusals ----

def _no_open(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a file was opened")
    monkeypatch.setattr("builtins.open", refuse)
    monkeypatch.setattr("gzip.open", refuse)


@pytest.mark.parametrize("kw,msg", [
    ({"infile": []}, "takes 1 to 64"),
    ({"infile": [f"s{k}.clonotypes.tsv" for k in range(65)]}, "takes 1 to 64"),
    ({"infile": ["x/a.clonotypes.tsv", "y/a.clonotypes.tsv.gz"]}, "two files give one sample name"),
    ({"metaclonotypes": None}, r"takes the meta-clonotypes \(-mc\)"),
    ({"cdr3_gap_cost": 0}, "--cdr3-gap-cost is 1 to 255"),
    ({"cdr3_gap_cost": 256}, "--cdr3-gap-cost is 1 to 255"),
    ({"cdr3_trim": "17,0"}, "--cdr3-trim is N,C"),
    ({"cdr3_trim": "3"}, "--cdr3-trim is N,C"),
    ({"cdr3_class": "j"}, "--cdr3-class is none, v or vj"),
])
def test_refusals_before_anything_is_opened(monkeypatch, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="tabulate", infile=["a.clonotypes.tsv"], metaclonotypes="mc.tsv", outpath="", prefix="", dontgzip=True)
    inp.update(kw)
    assert re.search(msg, tb.refusal(inp))
    with pytest.raises(ValueError, match=msg):
        tb.run(inp)


def test_the_limits_pass():
    base = dict(infile=["a.clonotypes.tsv"], metaclonotypes="mc.tsv")
    for kw in ({}, {"infile": [f"s{k}.clonotypes.tsv" for k in range(64)]}, {"cdr3_gap_cost": 255}, {"cdr3_trim": "16,16"}, {"cdr3_class": "vj"}):
        assert tb.refusal(dict(base, **kw)) is None, kw


@pytest.mark.parametrize("cell", [b"-1", b"70000", b"x", b"65536", b"3.0", b""])
def test_a_radius_that_is_no_radius_names_its_line(tmp_path, monkeypatch, cell):
    mc = MC.replace(b"CASSVRSSYEQYF\t5\t12\t", b"CASSVRSSYEQYF\t5\t" + cell + b"\t")
    assert mc != MC
    files, path = write_inputs(tmp_path, [("S1", S1)], mc)
    with pytest.raises(ValueError, match=r"A\.cdr3_metaclonotypes\.tsv, line 3: the radius .* is not an integer 0\.\.65535"):
        stage(tmp_path, monkeypatch, files, path)


def test_the_radius_limits_pass(tmp_path, monkeypatch):
    mc = MC.replace(b"CASSVRSSYEQYF\t5\t12\t", b"CASSVRSSYEQYF\t5\t65535\t").replace(b"CASSIRSSYEQYF\t10\t3\t", b"CASSIRSSYEQYF\t10\t0\t")
    files, path = write_inputs(tmp_path, [("S1", S1)], mc)
    res, _ = stage(tmp_path, monkeypatch, files, path)
    assert open(res["tabulate"], "rb").read().splitlines()[1:3] == [b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t0\t1\t1\t10",
                                                                   b"1\tTRBV1*01\tTRBJ1*01\tCASSVRSSYEQYF\t65535\t1\t3\t18"]


def test_a_missing_column_is_refused_by_its_flag(tmp_path, monkeypatch):
    files, mc = write_inputs(tmp_path, [("S1", S1)])
    for flag, option in (("mc_cdr3_column", "--mc-cdr3-column"), ("mc_v_column", "--mc-v-column"), ("mc_radius_column", "--mc-radius-column")):
        with pytest.raises(ValueError, match=r"no column 'nope' \(" + option + r"\)"):
            stage(tmp_path, monkeypatch, files, mc, **{flag: "nope"})
    with pytest.raises(ValueError, match=r"no column 'nope' \(--mc-j-column\)"):
        stage(tmp_path, monkeypatch, files, mc, mc_j_column="nope", cdr3_class="vj")
    res, _ = stage(tmp_path, monkeypatch, files, mc, mc_j_column="nope")      # (class v: not needed, not read)
    assert open(res["tabulate"], "rb").read().splitlines()[1] == b"0\tTRBV1*01\t\tCASSIRSSYEQYF\t3\t1\t2\t15"


def test_a_bad_cost_matrix_and_a_file_that_is_no_table_are_refused(tmp_path, monkeypatch):
    files, mc = write_inputs(tmp_path, [("S1", S1)])
    bad = str(tmp_path / "m.tsv")
    with open(bad, "wb") as fh:
        fh.write(b"\tA\tC\nA\t0\t1\nC\t2\t0\n")
    with pytest.raises(ValueError, match="m.tsv, line"):
        stage(tmp_path, monkeypatch, files, mc, cdr3_cost_matrix=bad)
    with pytest.raises(ValueError, match="is not a .clonotypes.tsv"):
        stage(tmp_path, monkeypatch, [mc], mc)


def test_refusals_from_the_command_line_and_the_parser(monkeypatch, capsys):
    from decombinator_amd.io import cli_args
    _no_open(monkeypatch)
    base = ["tabulate", "-in", "a.clonotypes.tsv", "-mc", "mc.tsv"]
    for words, msg in ((base + ["--cdr3-gap-cost", "0"], "--cdr3-gap-cost"), (base + ["--cdr3-trim", "x"], "--cdr3-trim"),
                       (base[:3], "takes the meta-clonotypes"), (base + ["-in", "b/a.clonotypes.tsv", "a.clonotypes.tsv"], "one sample name")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(words)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    inp = cli_args(base)
    assert inp["command"] == "tabulate" and inp["metaclonotypes"] == "mc.tsv" and inp["infile"] == ["a.clonotypes.tsv"]
    assert (inp["mc_cdr3_column"], inp["mc_v_column"], inp["mc_j_column"], inp["mc_radius_column"]) == ("junction_aa", "v_call", "j_call", "radius")
    assert (inp["cdr3_class"], inp["strip_alleles"], inp["prefix"], inp["dontgzip"]) == ("v", False, "dcr_", False) and tb.refusal(inp) is None
    inp = cli_args(base + ["--mc-radius-column", "r", "--cdr3-gap-cost", "8", "--cdr3-trim", "4,3", "--cdr3-cost-matrix", "m.tsv", "--cdr3-class", "vj", "-dz"])
    assert tb.refusal(inp) is None and inp["mc_radius_column"] == "r" and inp["cdr3_class"] == "vj" and inp["dontgzip"]


# ---- help ----

def test_help_names_every_flag_and_the_sub_command_list_stays():
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, "-m", "decombinator_amd", "tabulate", "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert got.returncode == 0
    for flag in ("-in", "-mc", "-op", "-pf", "-dz", "--mc-cdr3-column", "--mc-v-column", "--mc-j-column", "--mc-radius-column", "--cdr3-class",
                 "--strip-alleles", "--cdr3-gap-cost", "--cdr3-trim", "--cdr3-cost-matrix"):
        assert flag in got.stdout, flag
    assert "have to be the ones the meta-clonotypes were made under" in " ".join(got.stdout.split()).replace("- ", "-")      # (a line may break at a hyphen)
    assert "HAVE TO BE THE ONES THE META-CLONOTYPES WERE MADE UNDER" in " ".join(tb.__doc__.split())
    from decombinator_amd.io import create_parser
    choices = [a.choices for a in create_parser()._actions if getattr(a, "choices", None)]
    assert [list(c) for c in choices] == [["pipeline", "decombine", "collapse", "translate", "overlap"]]
    epilog = create_parser().epilog
    assert all(word in epilog for word in ("tabulate", "metaclonotypes", "motifs", "match"))
