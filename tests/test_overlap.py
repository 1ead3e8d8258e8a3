"""The `overlap` sub-command without a GPU: the per-row and per-pair code of dcrx_overlap_core.h against Python (host build),
the stage (decombinator_amd/overlap.py) with the contract's brute force standing in for _native.overlap, the host formatter,
the other sub-commands' help, and the ABI version."""
import ctypes as C
import gzip
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import overlap as ov
from decombinator_amd import pipeline
from tests import overlap_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELP_DIR = os.path.join(ROOT, "tests", "golden", "overlap_help")


# ---- the core header ----

def test_core_constants():
    h = ou.host_lib()
    assert h.overlap_host_max_samples() == nat.OVERLAP_MAX_SAMPLES == 64
    assert 1 << h.overlap_host_sample_bits() == 64
    assert h.overlap_host_planes() == len(nat.OVERLAP_PLANES) == 5


def test_full_compare_exhaustively_on_small_cases():
    h = ou.host_lib()
    keys = [(c, bytes(s)) for c in (0, 1, 0xFFFFFFFF) for n in range(4) for s in itertools.product(b"A\x00\xff", repeat=n)]
    for (ca, a), (cb, b) in itertools.product(keys, repeat=2):
        assert bool(h.overlap_host_equal(ca, a, len(a), cb, b, len(b))) == ((ca, a) == (cb, b)), (ca, a, cb, b)
    assert not h.overlap_host_equal(0, b"CASS", 4, 0, b"CASSL", 5)      # the length is part of the key
    assert not h.overlap_host_equal(0, b"CASS\x00", 5, 0, b"CASS", 4)


def test_plane_indices_exhaustively():
    h = ou.host_lib()
    for S in (1, 2, 3, 8, 63, 64):
        assert h.overlap_host_tri_size(S) == S * (S + 1) // 2
        full = [h.overlap_host_full_index(S, a, b) for a in range(S) for b in range(S)]
        assert full == list(range(S * S))                              # row major, every entry once
        tri = {}
        for a in range(S):
            for b in range(S):
                t = h.overlap_host_tri_index(a, b)
                assert t == h.overlap_host_tri_index(b, a) and t < S * (S + 1) // 2
                tri.setdefault(t, set()).add(frozenset((a, b)))
        assert len(tri) == S * (S + 1) // 2 and all(len(v) == 1 for v in tri.values())      # one place per unordered pair
    for g, a in ((0, 0), (1, 63), ((1 << 30) - 1, 63), (12345, 7)):
        k = h.overlap_host_cell_key(g, a)
        assert k >> 6 == g and k & 63 == a and k < 1 << 36


def test_product_split():
    h = ou.host_lib()
    top = (1 << 32) - 1
    rnd = random.Random(11)
    cases = [(0, 0), (0, top), (1, 1), (1, top), (top, top), (1 << 16, 1 << 16), (1 << 31, 2)]
    cases += [(rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(10000)]
    lo, hi = C.c_uint64(), C.c_uint64()
    for a, b in cases:
        h.overlap_host_product(a, b, C.byref(lo), C.byref(hi))
        assert (lo.value, hi.value) == ((a * b) % (1 << 32), (a * b) >> 32), (a, b)
        assert (hi.value << 32) + lo.value == a * b


def test_equal_keys_hash_equal():
    h = ou.host_lib()
    rnd = random.Random(5)
    seen = {}
    for _ in range(2000):
        c = rnd.choice((0, 1, 7, 0xFFFFFFFF))
        s = bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 40)))
        x = h.overlap_host_hash(c, s + b"tail", len(s))      # (only len bytes are read)
        assert x == h.overlap_host_hash(c, bytes(s), len(s))
        seen.setdefault(x, set()).add((c, s))
    assert len(seen) > 1900      # a filter that filters: nearly every key has a hash of its own
    assert h.overlap_host_hash(0, b"CASS", 4) != h.overlap_host_hash(1, b"CASS", 4)
    assert h.overlap_host_hash(0, b"CASS", 4) != h.overlap_host_hash(0, b"CASSL", 5)


# ---- the pair kernel's walk on the host: the look-ups the kernel's lanes make (first_above, group_end), around them the
# tiles, the staged ends, the per-block planes and the flush as plain loops (tests/host_overlap: overlap_host_pairs) ----

def _flat(planes):
    return [x for p in planes for r in p for x in r]


def test_the_constructed_lists_meet_their_premises():
    """What tests/test_gpu_overlap.py asserts before every device call, here where no device is needed."""
    for S in ou.PLANE_SIZES:
        groups, _, want = ou.constructed(f"plane_size_{S}")
        ou.premise_plane_size(groups, S, want)
    ou.premise_several_tiles(*ou.constructed("several_tiles"))
    for name in ou.LOOKUP_NAMES:
        ou.premise_lookup(name, ou.constructed("lookup_" + name)[0])
    for front in ou.TILE_EDGE_FRONTS:
        ou.premise_tile_edge(front, ou.constructed(f"tile_edge_{front}")[0])
    ou.premise_tile_edge_long(ou.constructed("tile_edge_long")[0])
    groups, _, want = ou.constructed("limit_weights")
    ou.premise_limit_weights(groups, want)
    groups, _, want = ou.constructed("one_entry")
    ou.premise_one_entry(groups, want)
    assert [ou.pairs_smax(S) for S in ou.PLANE_SIZES] == [8, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64]


@pytest.mark.parametrize("name", list(ou.CONSTRUCTED))
def test_host_walk_on_constructed_cells(name):
    groups, S, want = ou.constructed(name)
    smax = ou.pairs_smax(S)
    for grid in (1, 3, ou.PAIR_GRID):
        assert _flat(ou.host_pairs(groups, S, smax, grid)) == _flat(want), grid
    for larger in {x for x in (16, 64) if x > smax}:      # planes larger than the call needs: S, not SMAX, places an entry
        assert _flat(ou.host_pairs(groups, S, larger, 3)) == _flat(want), larger
    if smax == 64:
        assert ou.host_lib().overlap_host_pairs(len(groups), None, None, None, S, 32, 1, None) == -1      # smaller ones are refused


def test_host_walk_adds_onto_what_is_there():
    groups, S, _ = ou.constructed("plane_size_17")
    start = [[[1000 * (p * S * S + a * S + b) + 17 for b in range(S)] for a in range(S)] for p in range(5)]
    want = ou.expected_planes(groups, S, ou.expected_planes(groups, S, start))
    got = ou.host_pairs(groups, S, 32, 3, ou.host_pairs(groups, S, 32, 3, start))
    assert _flat(got) == _flat(want)


# ---- the stage, with the brute force in _native.overlap's place ----

A_ROWS = [("TRBV1", "TRBJ1", "CASSA", 10), ("TRBV1", "TRBJ1", "CASSB", 5), ("TRBV2", "TRBJ1", "CASSA", 1)]
B_ROWS = [("TRBV1", "TRBJ1", "CASSA", 20), ("TRBV1", "TRBJ1", "CASSC", 4)]
C_ROWS = [("TRBV1", "TRBJ1", "CASSA", 30), ("TRBV1", "TRBJ1", "CASSB", 5), ("TRBV2", "TRBJ2", "CASSD", 7)]

# Under vj the clonotypes are  V1 J1 CASSA: A 10, B 20, C 30;  V1 J1 CASSB: A 5, C 5;  and three private ones (A 1, B 4, C 7).
# Clonotypes n: A 3, B 2, C 3.  Reads X: A 16, B 24, C 42.  Sums of squares: A 100 + 25 + 1 = 126, B 400 + 16 = 416,
# C 900 + 25 + 49 = 974.
# A, B share CASSA: s = 1, reads 10 and 20, sum min = 10.  Jaccard 1 / (3 + 2 - 1) = 0.25; overlap coefficient 1 / 2;
#   Bray-Curtis 2 * 10 / (16 + 24) = 0.5; Morisita-Horn 2 * 200 * 16 * 24 / (126 * 24^2 + 416 * 16^2) = 153600 / 179072.
# A, C share CASSA and CASSB: s = 2, reads 15 and 35, sum min = 10 + 5.  Jaccard 2 / (3 + 3 - 2) = 0.5; 2 / 3;
#   2 * 15 / (16 + 42) = 30 / 58; 2 * (300 + 25) * 16 * 42 / (126 * 42^2 + 974 * 16^2) = 436800 / 471608.
# B, C share CASSA: s = 1, reads 20 and 30, sum min = 20.  1 / (2 + 3 - 1) = 0.25; 1 / 2; 40 / 66;
#   2 * 600 * 24 * 42 / (416 * 42^2 + 974 * 24^2) = 1209600 / 1294848.
HAND_PAIRS = (
    "sample_a\tsample_b\tclonotypes_a\tclonotypes_b\tshared_clonotypes\treads_a\treads_b\tshared_reads_a\tshared_reads_b\tmin_reads\t"
    "jaccard\toverlap_coefficient\tbray_curtis\tmorisita_horn\n"
    "A\tB\t3\t2\t1\t16\t24\t10\t20\t10\t0.250000\t0.500000\t0.500000\t0.857756\n"
    "A\tC\t3\t3\t2\t16\t42\t15\t35\t15\t0.500000\t0.666667\t0.517241\t0.926193\n"
    "B\tC\t2\t3\t1\t24\t42\t20\t30\t20\t0.250000\t0.500000\t0.606061\t0.934164\n").encode()
HAND_PUBLIC = (
    "v_call\tj_call\tjunction_aa\tn_samples\tduplicate_count\tA\tB\tC\n"
    "TRBV1\tTRBJ1\tCASSA\t3\t60\t10\t20\t30\n"
    "TRBV1\tTRBJ1\tCASSB\t2\t10\t5\t0\t5\n").encode()


def write_inputs(tmp_path, tables, gz=()):
    files = []
    for name, rows in tables:
        path = str(tmp_path / (name + ".clonotypes.tsv" + (".gz" if name in gz else "")))
        with (gzip.open if name in gz else open)(path, "wb") as fh:
            fh.write(ou.clonotypes_text(rows))
        files.append(path)
    return files


def stage(tmp_path, monkeypatch, files, calls=None, **kw):
    monkeypatch.setattr(nat, "overlap", ou.brute_force_native(calls))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out, exist_ok=True)
    inp = dict(command="overlap", infile=files, outpath=out, prefix="t_", dontgzip=True, overlap_key="vj", min_samples=2)
    inp.update(kw)
    res = ov.run(inp)
    read = lambda p: (gzip.open if p.endswith(".gz") else open)(p, "rb").read()
    return read(res["pairs"]), read(res["public"]), res


HAND = [("A", A_ROWS), ("B", B_ROWS), ("C", C_ROWS)]


def test_hand_case_byte_for_byte(tmp_path, monkeypatch):
    calls = []
    pairs, public, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, HAND), calls)
    assert pairs == HAND_PAIRS
    assert public == HAND_PUBLIC
    assert os.path.basename(res["pairs"]) == "t_overlap_pairs.tsv" and os.path.basename(res["public"]) == "t_overlap_public.tsv"
    assert oct(os.stat(res["pairs"]).st_mode)[-3:] == "666"
    assert len(calls) == 1      # ONE call of _native.overlap
    samples, classes, strings, weights, S, min_samples = calls[0]
    assert samples == [0, 0, 0, 1, 1, 2, 2, 2] and S == 3 and min_samples == 2
    assert classes == [0, 0, 1, 0, 0, 0, 0, 2]      # numbered from the (v_call, j_call) strings over all files
    assert strings == [b"CASSA", b"CASSB", b"CASSA", b"CASSA", b"CASSC", b"CASSA", b"CASSB", b"CASSD"]
    assert weights == [10, 5, 1, 20, 4, 30, 5, 7]
    assert ov.stats["groups"] == 5 and ov.stats["private_groups"] == 3 and ov.stats["in_all_samples"] == 1


def test_gzipped_inputs_and_outputs(tmp_path, monkeypatch):
    files = write_inputs(tmp_path, HAND, gz=("B", "C"))
    assert files[1].endswith(".gz") and files[0].endswith(".tsv")
    pairs, public, res = stage(tmp_path, monkeypatch, files, dontgzip=False)
    assert res["pairs"].endswith("overlap_pairs.tsv.gz") and res["public"].endswith("overlap_public.tsv.gz")
    assert pairs == HAND_PAIRS and public == HAND_PUBLIC


@pytest.mark.parametrize("mode", ["vj", "v", "none"])
def test_overlap_key(tmp_path, monkeypatch, mode):
    calls = []
    pairs, public, _ = stage(tmp_path, monkeypatch, write_inputs(tmp_path, HAND), calls, overlap_key=mode)
    v = [r[0] for _, rows in HAND for r in rows]
    j = [r[1] for _, rows in HAND for r in rows]
    assert calls[0][1] == ou.call_classes(v, j, mode)
    lines = public.decode().splitlines()
    if mode == "vj":
        assert public == HAND_PUBLIC
    elif mode == "v":      # nothing changes here but the classes' numbers: no two rows differ in the J call alone
        assert public == HAND_PUBLIC and calls[0][1] == [0, 0, 1, 0, 0, 0, 0, 1]
    else:                  # CASSA of TRBV2 joins the other CASSA: sample A's two rows add (10 + 1); the head row's calls are written
        assert lines[1] == "TRBV1\tTRBJ1\tCASSA\t3\t61\t11\t20\t30"
        assert pairs.decode().splitlines()[1].split("\t")[2:5] == ["2", "2", "1"]


def test_min_samples(tmp_path, monkeypatch):
    files = write_inputs(tmp_path, HAND)
    _, public, _ = stage(tmp_path, monkeypatch, files, min_samples=3)
    assert public == b"\n".join(HAND_PUBLIC.split(b"\n")[:2]) + b"\n"
    _, public, _ = stage(tmp_path, monkeypatch, files, min_samples=1)
    rows = [ln.split("\t") for ln in public.decode().splitlines()[1:]]
    assert len(rows) == 5
    # n_samples descending, then reads descending, then the first row's rank: C's CASSD (7), B's CASSC (4), A's TRBV2 CASSA (1)
    assert [(r[2], r[3], r[4]) for r in rows] == [("CASSA", "3", "60"), ("CASSB", "2", "10"), ("CASSD", "1", "7"), ("CASSC", "1", "4"),
                                                   ("CASSA", "1", "1")]
    assert rows[4][:2] == ["TRBV2", "TRBJ1"] and rows[4][5:] == ["1", "0", "0"]


def _no_open(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a file was opened before the refusal")
    monkeypatch.setattr(ov, "read_table", boom)
    monkeypatch.setattr(nat, "overlap", boom)


@pytest.mark.parametrize("files,kw,msg", [
    ([], {}, "1 to 64"),
    ([f"s{k}.clonotypes.tsv" for k in range(65)], {}, "1 to 64"),
    (["x/a.clonotypes.tsv", "y/a.clonotypes.tsv.gz"], {}, "one sample name"),
    (["a.clonotypes.tsv", "b.clonotypes.tsv"], {"min_samples": 0}, "--min-samples"),
    (["a.clonotypes.tsv", "b.clonotypes.tsv"], {"min_samples": 3}, "--min-samples"),
])
def test_refusals_before_anything_is_opened(monkeypatch, files, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="overlap", infile=files, outpath="", prefix="", dontgzip=True, overlap_key="vj", min_samples=2)
    inp.update(kw)
    assert msg in ov.refusal(inp)
    with pytest.raises(ValueError, match=msg):
        ov.run(inp)


def test_refusal_from_the_command_line(monkeypatch, capsys):
    _no_open(monkeypatch)
    with pytest.raises(SystemExit) as e:
        pipeline.main(["overlap", "-in", "a.clonotypes.tsv", "b.clonotypes.tsv", "--min-samples", "5"])
    assert e.value.code == 2 and "--min-samples" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pipeline.main(["overlap", "-in", "a.clonotypes.tsv", "--overlap-key", "j"])


def test_sample_names():
    assert ov.sample_name("/x/y/dcr_S1_beta.clonotypes.tsv.gz") == "dcr_S1_beta"
    assert ov.sample_name("S2.clonotypes.tsv") == "S2"
    assert ov.sample_name("other.tsv") == "other.tsv"


def test_wrong_header_is_refused(tmp_path, monkeypatch):
    bad = tmp_path / "bad.clonotypes.tsv"
    bad.write_bytes(b"v_call\tj_call\tjunction_aa\tcount\nTRBV1\tTRBJ1\tCASS\t3\n")
    good = write_inputs(tmp_path, HAND[:1])
    with pytest.raises(ValueError, match="not a .clonotypes.tsv"):
        stage(tmp_path, monkeypatch, good + [str(bad)])
    empty = tmp_path / "empty.clonotypes.tsv"
    empty.write_bytes(b"")
    with pytest.raises(ValueError, match="not a .clonotypes.tsv"):
        stage(tmp_path, monkeypatch, [str(empty)], min_samples=1)


def test_one_sample(tmp_path, monkeypatch):
    pairs, public, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, HAND[:1]), min_samples=1)
    assert pairs == HAND_PAIRS.split(b"\n")[0] + b"\n"      # the header alone
    assert public.decode().splitlines() == ["v_call\tj_call\tjunction_aa\tn_samples\tduplicate_count\tA",
                                            "TRBV1\tTRBJ1\tCASSA\t1\t10\t10", "TRBV1\tTRBJ1\tCASSB\t1\t5\t5", "TRBV2\tTRBJ1\tCASSA\t1\t1\t1"]


def test_a_sample_with_a_header_only(tmp_path, monkeypatch):
    pairs, public, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, [("A", A_ROWS), ("E", []), ("C", C_ROWS)]))
    lines = [ln.split("\t") for ln in pairs.decode().splitlines()]
    assert [ln[:2] for ln in lines[1:]] == [["A", "E"], ["A", "C"], ["E", "C"]]
    assert lines[1][2:10] == ["3", "0", "0", "16", "0", "0", "0", "0"]
    assert lines[1][10:] == ["0.000000", "nan", "0.000000", "nan"]      # 0 / 3; 0 / min(3, 0); 0 / 16; 0 / (126 * 0 + 0 * 256)
    assert lines[2][10:] == HAND_PAIRS.decode().splitlines()[2].split("\t")[10:]
    assert res["stats"]["rows_per_sample"] == [3, 0, 3]
    assert public.decode().splitlines()[1] == "TRBV1\tTRBJ1\tCASSA\t2\t40\t10\t0\t30"
    # every file a header only: no rows at all
    pairs, public, res = stage(tmp_path, monkeypatch, write_inputs(tmp_path, [("E", []), ("F", [])]))
    assert pairs.decode().splitlines()[1].split("\t")[10:] == ["nan"] * 4 and len(public.splitlines()) == 1
    assert res["stats"]["rows_in"] == 0


# ---- the host formatter ----

def test_format_overlap_public_against_python():
    samples, v, j, s, w = ou.random_tables(5, 300, 200, seed=3)
    s[7] = ""                                  # an empty string is a key like any other
    s[11] = "CA\x80\xffSS"                     # bytes >= 0x80 are written as they are
    names = ["s0", "sample one", "s2", "sé", "s4"]
    for mode, min_samples in (("vj", 2), ("none", 1), ("v", 5)):
        result, _ = ou.expected_overlap(samples, ou.call_classes(v, j, mode), s, w, 5, min_samples)
        v_calls, j_calls = sorted(set(v)), sorted(set(j))
        off, text = ou.row_text(s)
        got = nat.format_overlap_public(result, names, [v_calls.index(x) for x in v], [j_calls.index(x) for x in j], v_calls, j_calls,
                                        off, text)
        want = ou.public_text(result, [n.encode("utf-8").decode("latin-1") for n in names], v, j, s)
        assert got == want, mode
        assert len(result["head"]) > 0


def test_format_overlap_public_refuses_what_does_not_fit():
    result, _ = ou.expected_overlap([0, 1], [0, 0], ["CASS", "CASS"], [1, 2], 2)
    off, text = ou.row_text(["CASS", "CASS"])
    with pytest.raises(nat.DcrxError):       # a head outside the rows
        nat.format_overlap_public(dict(result, head=np.array([9], np.uint32)), ["a", "b"], [0, 0], [0, 0], ["V"], ["J"], off, text)
    with pytest.raises(nat.DcrxError):       # a cell's sample outside the names
        nat.format_overlap_public(result, ["a"], [0, 0], [0, 0], ["V"], ["J"], off, text)


# ---- what must not have changed ----

@pytest.mark.parametrize("command", ["decombine", "pipeline", "translate"])
def test_other_help_texts_are_unchanged(command):
    env = dict(os.environ, COLUMNS="100", PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, "-m", "decombinator_amd", command, "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert got.returncode == 0
    want = open(os.path.join(HELP_DIR, command + ".txt")).read()      # the text before `overlap` existed
    assert got.stdout.split() == want.split()


def test_list_of_sub_commands_gains_one():
    from decombinator_amd.io import create_parser
    text = create_parser().format_help()
    assert "{pipeline,decombine,collapse,translate,overlap}" in text
    sub = [a for a in create_parser()._actions if getattr(a, "choices", None) and "overlap" in a.choices][0]
    assert list(sub.choices) == ["pipeline", "decombine", "collapse", "translate", "overlap"]


def test_abi_version_is_5():
    assert nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and "#define DCRX_OVERLAP_MAX_SAMPLES 64" in hdr


def test_host_entries_refuse_without_a_device():
    """The argument checks of dcrx_overlap_run come before anything touches a device, and m = 0 touches none."""
    one = np.zeros(1, np.uint32)
    for S in (0, 65):
        with pytest.raises(nat.DcrxError) as e:
            nat.overlap(one[:0], one[:0], np.zeros(1, np.uint64), b"", np.zeros(0, np.uint64), S, 1)
        assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:
        nat.overlap(one[:0], one[:0], np.zeros(1, np.uint64), b"", np.zeros(0, np.uint64), 2, 0)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:      # a sample id equal to S
        nat.overlap([2], [0], [0, 4], b"CASS", [1], 2, 1)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:      # offsets going backwards
        nat.overlap([0, 0], [0, 0], [4, 2, 4], b"CASS", [1, 1], 2, 1)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:      # a row of weight 2^32
        nat.overlap([0], [0], [0, 4], b"CASS", [1 << 32], 2, 1)
    assert e.value.code == -2
    got = nat.overlap(one[:0], one[:0], np.zeros(1, np.uint64), b"", np.zeros(0, np.uint64), 3, 2)
    ou.assert_same(got, ou.expected_overlap([], [], [], [], 3, 2), [])
    with pytest.raises(nat.DcrxError):
        nat.overlap_set_hash_bits(65)
