"""`match --cdr3-metric weighted` (include/dcrx.h "match, weighted") without a GPU: the default table, every refusal of the C
entries and of the sub-command, the matrix-file reader, the pair test of the shared header against the contract in Python
(tests/cdr3_wmatch_util.py), the host walk of the kernel's steps on the constructed lists, the host formatter, the stage over a
stubbed native call, and the stand-alone sanitizer run of the host walk."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import match as mt
from decombinator_amd import pipeline
from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu
from tests.test_cdr3_match import A_ROWS, DB, DB_FLAGS, write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the default table ----

NEAR = {9: "AS RQ ND NH NS QK EK IM LV MV FW ST", 6: "RK DE QE HY IL LM WY", 3: "IV FY"}


def test_default_table_is_symmetric_zero_on_the_diagonal_and_holds_the_21_pairs():
    cost = nat.Cdr3Cost.default()
    sub = cost.sub.astype(int)
    assert (cost.gap, cost.ntrim, cost.ctrim) == (12, 3, 2) and sub.shape == (32, 32)
    assert (sub == sub.T).all() and not sub.diagonal().any()
    want = {frozenset(p): c for c, pairs in NEAR.items() for p in pairs.split()}
    assert len(want) == 21
    for x, y in itertools.combinations(range(1, 27), 2):
        assert sub[x, y] == want.get(frozenset(chr(64 + x) + chr(64 + y)), 12), (chr(64 + x), chr(64 + y))
    assert not sub[0].any() and not sub[27:].any() and not sub[:, 27:].any()
    assert all(sub[ord(x) & 31, ord(y) & 31] == 12 for x in "BJOUXZ" for y in "ACDEFGHIKLMNPQRSTVWYBJOUXZ" if x != y)


# ---- refusals of the C entries: on the host, before any device call (an index of no targets touches no device) ----

def _empty_index():
    return nat.Cdr3Index(np.zeros(0, np.uint32), np.zeros(1, np.uint64), b"")


def _bad_costs():
    ok = nat.Cdr3Cost.default()
    asym, diag = ok.sub.copy(), ok.sub.copy()
    asym[1, 3] = 5
    diag[26, 26] = 1
    return [(nat.Cdr3Cost(asym), 24, "symmetric"), (nat.Cdr3Cost(diag), 24, "diagonal"), (nat.Cdr3Cost.default(gap=0), 24, "gap"),
            (nat.Cdr3Cost.default(gap=256), 24, "gap"), (nat.Cdr3Cost.default(ntrim=17), 24, "trim"),
            (nat.Cdr3Cost.default(ctrim=17), 24, "trim"), (ok, 65536, "radius"), (None, 24, "null cost")]


def test_the_weighted_entries_refuse_what_the_contract_refuses():
    index = _empty_index()
    q = (np.zeros(1, np.uint32), np.array([0, 5], np.uint64), b"CASSF", np.ones(1, np.uint64))
    try:
        for cost, radius, msg in _bad_costs():
            with pytest.raises(nat.DcrxError, match=msg) as e:
                nat.cdr3_match_weighted(index, *q, cost, radius)
            assert e.value.code == -1
            with pytest.raises(nat.DcrxError, match=msg):
                nat.cdr3_match_weighted_device(index, 0, None, None, None, 0, cost, radius, None, None, None, None, 0, None, None, 0)
            if cost is not None and radius <= 65535:
                with pytest.raises(nat.DcrxError, match=msg):
                    nat.format_cdr3_matches_weighted({"hit_off": np.zeros(1, np.uint64), "hit": []}, [], [], [], [], np.zeros(1, np.uint64), b"",
                                                     [], np.zeros(1, np.uint64), b"", b"db_x", [], cost)
        # the table's unread rows and columns may hold anything; the limits themselves pass
        loose = nat.Cdr3Cost.default(gap=255, ntrim=16, ctrim=16)
        loose.sub[0, 5], loose.sub[27, 1], loose.sub[3, 31] = 9, 8, 7
        got = nat.cdr3_match_weighted(index, *q, loose, 65535)
        assert got["stats"]["hits"] == 0 and got["stats"]["queries"] == 1 and len(got["hit_dist"]) == 0
        with pytest.raises(nat.DcrxError, match="2\\^64"):
            nat.cdr3_match_weighted(index, np.zeros(2, np.uint32), np.array([0, 5, 5], np.uint64), b"CASSF",
                                    np.array([(1 << 64) - 1, 1], np.uint64), nat.Cdr3Cost.default(), 24)
        assert nat.cdr3_match_weighted(index, np.zeros(2, np.uint32), np.array([0, 5, 5], np.uint64), b"CASSF",
                                       np.array([(1 << 64) - 2, 1], np.uint64), nat.Cdr3Cost.default(), 24)["stats"]["queries"] == 2
        assert nat.cdr3_match_weighted_work_bytes(1 << 30, 0) == 0
        assert nat.cdr3_match_weighted_work_bytes(1000, 0) == nat.cdr3_match_work_bytes(1000, 0, "hamming")
    finally:
        index.close()


def test_the_old_entries_still_refuse_metric_2_and_export_dist_serves_weighted_handles_alone():
    L = nat.lib()
    assert nat.CDR3_METRICS == {"hamming": 0, "levenshtein": 1} and nat.CDR3_METRIC_WEIGHTED == 2
    assert L.dcrx_cdr3_match_work_bytes(10, 0, 2) == 0
    index = _empty_index()
    try:
        cls, off, w = np.zeros(1, np.uint32), np.array([0, 5], np.uint64), np.ones(1, np.uint64)
        text = np.frombuffer(b"CASSF\0", np.uint8)
        h = C.c_void_p()
        assert L.dcrx_cdr3_match_run(index.handle, 1, cls.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data, 1, 2, C.byref(h)) == -1
        assert not h.value and b"metric" in L.dcrx_last_error()
        assert L.dcrx_cdr3_match_device(index.handle, 0, None, None, None, 0, 1, 2, None, None, None, 0, None, None, 0, None) == -1
        assert L.dcrx_format_cdr3_matches(0, None, None, None, None, 0, None, None, 0, None, None, None, None, None, 0, None, None, None, 0,
                                          None, None, 2, None, 0) == -1
        assert L.dcrx_cdr3_match_run(index.handle, 1, cls.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data, 1, 0, C.byref(h)) == 0
        one = np.zeros(1, np.uint32)
        assert L.dcrx_cdr3_match_export_dist(h, one.ctypes.data) == -1 and b"weighted" in L.dcrx_last_error()
        L.dcrx_cdr3_match_destroy(h)
        assert L.dcrx_cdr3_match_export_dist(None, one.ctypes.data) == -1
        cost = nat.Cdr3Cost.default().as_c()
        assert L.dcrx_cdr3_match_weighted_run(index.handle, 1, cls.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data,
                                              C.addressof(cost), 24, C.byref(h)) == 0
        assert L.dcrx_cdr3_match_export_dist(h, None) == 0 and L.dcrx_cdr3_match_export_dist(h, one.ctypes.data) == 0
        L.dcrx_cdr3_match_destroy(h)
    finally:
        index.close()


def test_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "dcrx.h")).read()
    assert "#define DCRX_ABI_VERSION 5" in hdr and "#define DCRX_CDR3NET_WEIGHTED 2" in hdr
    for name in ("dcrx_cdr3_match_weighted_work_bytes", "dcrx_cdr3_match_weighted_device", "dcrx_cdr3_match_weighted_run",
                 "dcrx_cdr3_match_export_dist", "dcrx_format_cdr3_matches_weighted"):
        assert name in nat.EXPORTS and name + "(" in hdr and hasattr(nat.lib(), name)
    assert C.sizeof(nat.Cdr3CostC) == 1024 + 12


# ---- the matrix file ----

def _matrix_text(letters, cell) -> bytes:
    rows = ["\t".join(["."] + list(letters))]
    for x in letters:
        rows.append("\t".join([x] + [str(cell(x, y)) for y in letters]))
    return ("\n".join(rows) + "\n").encode()


def test_the_matrix_file_reader(tmp_path):
    path = str(tmp_path / "m.tsv")
    letters = nat.AMINO_ACIDS + "X"
    cell = lambda x, y: 0 if x == y else 1 + (ord(x) * ord(y)) % 40
    open(path, "wb").write(_matrix_text(letters, cell))
    cost = nat.Cdr3Cost.from_file(path, 7, 1, 0)
    assert (cost.gap, cost.ntrim, cost.ctrim) == (7, 1, 0)
    top = max(cell(x, y) for x in letters for y in letters)
    for x in "ACDEFGHIKLMNPQRSTVWYXBZ":
        for y in "ACDEFGHIKLMNPQRSTVWYXBZ":
            want = 0 if x == y else cell(x, y) if x in letters and y in letters else top      # a letter the file lacks: its largest cell
            assert cost.sub[ord(x) & 31, ord(y) & 31] == want, (x, y)
    assert not cost.sub[0].any() and not cost.sub[27:].any()
    open(path, "wb").write(_matrix_text(letters, cell).replace(b"\n", b"\r\n"))
    assert (nat.Cdr3Cost.from_file(path).sub == cost.sub).all()      # CRLF, and the default gap and trims
    # the default table written out and read back is the default table
    open(path, "wb").write(_matrix_text(nat.AMINO_ACIDS, lambda x, y: int(nat.Cdr3Cost.default_table()[ord(x) & 31, ord(y) & 31])))
    assert (nat.Cdr3Cost.from_file(path).sub == nat.Cdr3Cost.default_table()).all()


@pytest.mark.parametrize("edit,msg", [
    (lambda t: b"", "line 1"),
    (lambda t: t.replace(b"\tW", b"\tw", 1), "line 1: 'w'"),
    (lambda t: t.replace(b"\tW", b"\tWW", 1), "line 1: 'WW'"),
    (lambda t: t.replace(b".\tA\tC", b".\tA\tA", 1), "line 1: a letter stands twice"),
    (lambda t: b"\n".join(b"\t".join(ln.split(b"\t")[:-1]) for ln in t.split(b"\n")[:-2]) + b"\n", "line 1: no column for Y"),
    (lambda t: b"\n".join(t.split(b"\n")[:-2]) + b"\n", "line 20: 19 rows under 20 columns"),
    (lambda t: t.replace(b"\nD\t", b"\nE\t", 1), "line 4: row E where the header has D"),
    (lambda t: t.replace(b"\nD\t5", b"\nD\t256", 1), "line 4: '256'"),
    (lambda t: t.replace(b"\nD\t5", b"\nD\t-1", 1), "line 4: '-1'"),
    (lambda t: t.replace(b"\nD\t5", b"\nD\t6", 1), "line 4: D-A is 6 but A-D is 5"),
    (lambda t: t.replace(b"\nC\t5\t0", b"\nC\t5\t1", 1), "line 3: the diagonal cell is 1"),
    (lambda t: t.replace(b"\nD\t5\t5", b"\nD\t5", 1), "line 4: 20 fields, not 21"),
])
def test_a_bad_matrix_file_is_refused_by_its_line_before_any_device_call(tmp_path, monkeypatch, edit, msg):
    good = _matrix_text(nat.AMINO_ACIDS, lambda x, y: 0 if x == y else 5)
    path = str(tmp_path / "m.tsv")
    open(path, "wb").write(edit(good))
    with pytest.raises(ValueError, match=msg):
        nat.Cdr3Cost.from_file(path)

    def boom(*a, **k):
        raise AssertionError("the device was called, or a table read, before the refusal")
    for name in ("Cdr3Index", "cdr3_match_weighted"):
        monkeypatch.setattr(nat, name, boom)
    monkeypatch.setattr(mt, "read_table", boom)
    monkeypatch.setattr(mt, "read_database", boom)
    with pytest.raises(ValueError, match=msg):
        mt.run(dict(command="match", infile=["a.clonotypes.tsv"], database="db.tsv", outpath="", prefix="", dontgzip=True,
                    cdr3_metric="weighted", cdr3_cost_matrix=path))


# ---- the pair test of the shared header against the contract ----

SETTINGS = [(0, 0, 5, 20), (3, 2, 12, 24), (1, 4, 200, 65535), (2, 1, 1, 0)]      # (ntrim, ctrim, gap, R)


def _matrix(strings):
    m = np.zeros((len(strings), wu.MAX_LEN), np.uint8)
    for k, s in enumerate(strings):
        m[k, :len(s)] = np.frombuffer(s, np.uint8)
    return m


def test_weighted_within_on_all_pairs_of_short_strings_over_three_letters():
    """Every ordered pair (own, other) of the 3 280 strings of 0 .. 7 letters over {A, I, V}: weighted_within == min(dist, R + 1),
    dist by the literal minimum over every p as array operations (wu.group_dist, itself checked against wu.dist here)."""
    by_len = {L: [bytes(t) for t in itertools.product(b"AIV", repeat=L)] for L in range(8)}
    assert sum(len(v) for v in by_len.values()) == 3280
    rnd = random.Random(3)
    for seed, (ntrim, ctrim, gap, R) in enumerate(SETTINGS):
        cost = wu.random_cost(20 + seed, gap, ntrim, ctrim, top=40 if R < 100 else 255)
        for lo, lb in itertools.product(range(8), repeat=2):
            own, other = by_len[lo], by_len[lb]
            A, B = _matrix(own), _matrix(other)
            got = wu.host_within_grid(A, lo, B, lb, cost, R)
            a, b = ((A[:, None, :] & 31), (B[None, :, :] & 31)) if lo <= lb else ((B[None, :, :] & 31), (A[:, None, :] & 31))
            want = np.minimum(wu.group_dist(a, b, min(lo, lb), abs(lo - lb), cost), R + 1)
            assert got.shape == want.shape and np.array_equal(got, want), (lo, lb, ntrim, ctrim, gap, R)
            for _ in range(3):      # the array form is the literal one
                i, j = rnd.randrange(len(own)), rnd.randrange(len(other))
                assert min(wu.dist(own[i], other[j], cost), R + 1) == want[i, j]


def test_weighted_within_on_random_pairs_up_to_32_letters():
    """10^5 random pairs of 1 .. 32 letters — related pairs (a few substitutions and one block inserted) and unrelated ones."""
    rnd = random.Random(9)
    letters = "ACDEFGHIKLMNPQRSTVWYBXZ"
    pairs = []
    while len(pairs) < 100000:
        a = "".join(rnd.choice(letters) for _ in range(rnd.randrange(1, 33)))
        if rnd.random() < 0.7:
            b = list(a)
            for _ in range(rnd.randrange(4)):
                b[rnd.randrange(len(b))] = rnd.choice(letters)
            p, d = rnd.randrange(len(b) + 1), rnd.choice((0, 0, 1, 1, 2, 3, 8))
            b = "".join(b[:p]) + "".join(rnd.choice(letters) for _ in range(d)) + "".join(b[p:])
            b = b[:32]
        else:
            b = "".join(rnd.choice(letters) for _ in range(rnd.randrange(1, 33)))
        pairs.append((a.encode(), b.encode()) if rnd.random() < 0.5 else (b.encode(), a.encode()))
    A, B = _matrix([a for a, _ in pairs]), _matrix([b for _, b in pairs])
    la, lb = np.array([len(a) for a, _ in pairs]), np.array([len(b) for _, b in pairs])
    for seed, (ntrim, ctrim, gap, R) in enumerate([(3, 2, 12, 24), (0, 0, 7, 300), (16, 16, 255, 65535), (1, 1, 3, 0)]):
        cost = nat.Cdr3Cost.default(gap, ntrim, ctrim) if seed == 0 else wu.random_cost(40 + seed, gap, ntrim, ctrim)
        got = wu.host_within_many(pairs, cost, R)
        want = np.zeros(len(pairs), np.int64)
        for x, y in set(zip(la.tolist(), lb.tolist())):
            k = np.flatnonzero((la == x) & (lb == y))
            a, b = (A[k] & 31, B[k] & 31) if x <= y else (B[k] & 31, A[k] & 31)
            want[k] = wu.group_dist(a, b, min(x, y), abs(x - y), cost)
        assert np.array_equal(got, np.minimum(want, R + 1)), (ntrim, ctrim, gap, R)
        assert (want <= R).sum() > 100 or R == 0
        for k in range(0, len(pairs), 997):
            assert wu.dist(*pairs[k], cost) == want[k]


def test_the_plateaus_and_the_step_of_the_gap():
    """What a kernel may use: every p below ntrim costs what p = ntrim costs, every p above la - ctrim what p = la - ctrim costs,
    and moving the gap from p to p + 1 changes the sum by sub[a[p]][b[p]] - sub[a[p]][b[p + d]] at a counted p (by nothing at
    another)."""
    rnd = random.Random(4)
    for _ in range(300):
        ntrim, ctrim = rnd.randrange(0, 6), rnd.randrange(0, 6)
        cost = wu.random_cost(rnd.randrange(1000), 9, ntrim, ctrim)
        la, d = rnd.randrange(1, 20), rnd.randrange(1, 8)
        a = bytes(rnd.choice(wu.AMINO.encode()) for _ in range(la))
        b = bytes(rnd.choice(wu.AMINO.encode()) for _ in range(la + d))
        sums = [wu.gap_sum(a, b, p, cost) for p in range(la + 1)]
        if la > ntrim + ctrim:
            assert all(sums[p] == sums[ntrim] for p in range(ntrim)) and all(sums[p] == sums[la - ctrim] for p in range(la - ctrim, la + 1))
        else:
            assert not any(sums) and wu.dist(a, b, cost) == d * cost.gap
        for p in range(la):
            step = int(cost.sub[a[p] & 31, b[p] & 31]) - int(cost.sub[a[p] & 31, b[p + d] & 31]) if ntrim <= p < la - ctrim else 0
            assert sums[p + 1] - sums[p] == step


def test_letters_only_of_the_shared_header():
    rnd = random.Random(6)
    for L in range(1, 33):
        base = bytes(rnd.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(L))
        assert wu.host_letters(base)
        for p in {0, L - 1, rnd.randrange(L), (L - 1) // 4 * 4, min(L - 1, 3)}:
            for bad in (0x00, 0x40, 0x5B, 0x5F, 0x2A, 0x61, 0x7A, 0x7F, 0x80, 0xC1, 0xDA, 0xFF):
                assert not wu.host_letters(base[:p] + bytes([bad]) + base[p + 1:]), (L, p, bad)
    for b in range(256):
        assert wu.host_letters(bytes([b])) == (65 <= b <= 90)


# ---- the host walk of the kernel's steps ----

def test_host_walk_gives_the_contract_on_the_constructed_lists():
    lists = wu.constructed()
    assert len(lists) >= 60
    for name, (case, cost, R) in lists.items():
        want = wu.expected(case, cost, R)
        degree, hit_off, hit, hit_dist = wu.host_match(case, cost, R)
        for k, got in (("degree", degree), ("hit_off", hit_off), ("hit", hit), ("hit_dist", hit_dist)):
            assert np.array_equal(np.asarray(got, np.uint64), np.asarray(want[k], np.uint64)), (name, k)


def test_host_walk_and_the_numpy_form_on_random_families():
    ts, tv, tj, qs, qv, qj = mu.random_case(300, 700, 4, 2, seed=8, pool=260)
    case = mu.classed(ts, tv, tj, qs, qv, qj, "v")
    for cost, R in ((wu.default_cost(), 24), (wu.default_cost(), 12), (wu.random_cost(2, 5, 0, 1, top=30), 40)):
        want = wu.expected(case, cost, R)
        assert want["stats"]["hits"] > 100 and len(set(want["hit_dist"].tolist())) > 3
        wu.assert_same(wu.expected_numpy(case, cost, R), want)
        degree, hit_off, hit, hit_dist = wu.host_match(case, cost, R)
        assert np.array_equal(hit, want["hit"]) and np.array_equal(hit_dist, want["hit_dist"]) and np.array_equal(degree, want["degree"])


def test_sanitizer_run_of_the_host_walk():
    """The stand-alone program (its own main) under AddressSanitizer and UBSan: host code, on the CPU."""
    got = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_cdr3wmatch"), "asan"], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-2000:]
    assert got.stdout.strip().endswith("ok") and "rows differ" in got.stdout and "every length" in got.stdout


# ---- the host formatter ----

def test_format_cdr3_matches_weighted_against_python():
    ts, tv, tj, qs, qv, qj = mu.random_case(120, 150, 3, 2, seed=5)
    case = mu.classed(ts, tv, tj, qs, qv, qj, "v")
    db_header = [b"cdr3", b"v", b"epitope"]
    db_lines = [b"\t".join([t, v.encode(), b"EPI%d" % k]) for k, (t, v) in enumerate(zip(case.t_strings, tv))]
    q_off, q_text = cnu.node_text(case.q_strings)
    t_off, t_text = cnu.node_text(case.t_strings)
    v_calls, j_calls = sorted(set(qv)), sorted(set(qj))
    for cost, R in ((wu.default_cost(), 24), (wu.random_cost(1, 30, 2, 0), 200)):
        result = wu.expected(case, cost, R)
        assert result["stats"]["hits"] > 0 and any(d > 0 for d in result["hit_dist"].tolist())
        got = nat.format_cdr3_matches_weighted(result, [v_calls.index(x) for x in qv], [j_calls.index(x) for x in qj], v_calls, j_calls, q_off,
                                               q_text, case.weights, t_off, t_text, b"\t".join(b"db_" + h for h in db_header), db_lines, cost)
        assert got == wu.matches_text(qv, qj, case, result, db_header, db_lines, cost)
        assert [int(ln.split(b"\t")[6]) for ln in got.splitlines()[1:]] == result["hit_dist"].tolist()
    # a hit the metric cannot have: a byte outside A .. Z, a string out of reach
    bad = mu.Case([0, 0], ["CASsF", "C" * 33], [0], ["CASSF"], [1])
    o, t = cnu.node_text(bad.q_strings)
    to, tt = cnu.node_text(bad.t_strings)
    for j in (0, 1):
        with pytest.raises(nat.DcrxError, match="reach"):
            nat.format_cdr3_matches_weighted({"hit_off": np.array([0, 1], np.uint64), "hit": np.array([j], np.uint32)}, [0], [0], ["V"], ["J"],
                                             o, t, [1], to, tt, b"db_a", [b"x", b"y"], wu.default_cost())


# ---- the sub-command ----

def _no_open(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a file was opened, or the device called, before the refusal")
    monkeypatch.setattr(mt, "read_table", boom)
    monkeypatch.setattr(mt, "read_database", boom)
    for name in ("Cdr3Index", "cdr3_match", "cdr3_match_weighted"):
        monkeypatch.setattr(nat, name, boom)
    monkeypatch.setattr(nat.Cdr3Cost, "from_file", boom)


@pytest.mark.parametrize("kw,msg", [
    ({"cdr3_radius": 24}, "--cdr3-radius goes with --cdr3-metric weighted"),
    ({"cdr3_gap_cost": 12, "cdr3_metric": "levenshtein"}, "--cdr3-gap-cost goes with"),
    ({"cdr3_trim": "3,2"}, "--cdr3-trim goes with"),
    ({"cdr3_cost_matrix": "m.tsv", "cdr3_metric": "hamming"}, "--cdr3-cost-matrix goes with"),
    ({"cdr3_metric": "weighted", "cdr3_distance": 2}, "--cdr3-distance does not apply"),
    ({"cdr3_metric": "weighted", "cdr3_distance": 0}, "--cdr3-distance does not apply"),
    ({"cdr3_metric": "weighted", "cdr3_radius": 65536}, "--cdr3-radius is 0 to 65535"),
    ({"cdr3_metric": "weighted", "cdr3_radius": -1}, "--cdr3-radius is 0 to 65535"),
    ({"cdr3_metric": "weighted", "cdr3_trim": "17,2"}, "--cdr3-trim is N,C"),
    ({"cdr3_metric": "weighted", "cdr3_trim": "3,17"}, "--cdr3-trim is N,C"),
    ({"cdr3_metric": "weighted", "cdr3_trim": "3"}, "--cdr3-trim is N,C"),
    ({"cdr3_metric": "weighted", "cdr3_trim": "a,b"}, "--cdr3-trim is N,C"),
    ({"cdr3_metric": "weighted", "cdr3_gap_cost": 0}, "--cdr3-gap-cost is 1 to 255"),
    ({"cdr3_metric": "weighted", "cdr3_gap_cost": 256}, "--cdr3-gap-cost is 1 to 255"),
    ({"cdr3_metric": "tcrdist"}, "--cdr3-metric is one of hamming, levenshtein, weighted"),
])
def test_refusals_before_anything_is_opened(monkeypatch, kw, msg):
    _no_open(monkeypatch)
    inp = dict(command="match", infile=["a.clonotypes.tsv"], database="db.tsv", outpath="", prefix="", dontgzip=True)
    inp.update(kw)
    assert msg in mt.refusal(inp)
    with pytest.raises(ValueError, match=msg):
        mt.run(inp)


def test_refusals_from_the_command_line_and_the_parser(monkeypatch, capsys):
    from decombinator_amd.io import cli_args
    _no_open(monkeypatch)
    base = ["match", "-in", "a.clonotypes.tsv", "-db", "db.tsv"]
    for extra, msg in ((["--cdr3-radius", "30"], "--cdr3-radius goes with"),
                       (["--cdr3-metric", "weighted", "--cdr3-distance", "2"], "--cdr3-distance does not apply"),
                       (["--cdr3-metric", "weighted", "--cdr3-radius", "70000"], "--cdr3-radius is 0 to 65535"),
                       (["--cdr3-metric", "weighted", "--cdr3-trim", "20,0"], "--cdr3-trim")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    inp = cli_args(base)
    assert (inp["cdr3_metric"], inp["cdr3_radius"], inp["cdr3_gap_cost"], inp["cdr3_trim"], inp["cdr3_cost_matrix"]) == \
        ("hamming", None, None, None, None)
    inp = cli_args(base + ["--cdr3-metric", "weighted", "--cdr3-radius", "36", "--cdr3-gap-cost", "8", "--cdr3-trim", "4,3",
                           "--cdr3-cost-matrix", "m.tsv"])
    assert (inp["cdr3_metric"], inp["cdr3_radius"], inp["cdr3_gap_cost"], inp["cdr3_trim"], inp["cdr3_cost_matrix"]) == \
        ("weighted", 36, 8, "4,3", "m.tsv")
    assert mt.refusal(inp) is None
    cost, radius = mt.weighted_settings(dict(cdr3_metric="weighted"))
    assert (radius, cost.gap, cost.ntrim, cost.ctrim) == (24, 12, 3, 2) and (cost.sub == nat.Cdr3Cost.default_table()).all()


W_ROWS = [("TRBV1*01", "TRBJ1*01", "CASSIRSSYEQYF", 10), ("TRBV1*01", "TRBJ1*01", "CASSWRSSYEQYF", 5), ("TRBV1*01", "TRBJ1*01", "CASSIRSYEQYF", 3),
          ("TRBV1*01", "TRBJ1*01", "CASSIRSS*EQYF", 2), ("TRBV2*01", "TRBJ1*01", "CASSIRSSYEQYF", 1), ("TRBV1*01", "TRBJ1*01", "cassirssyeqyf", 7)]
W_DB = (b"CDR3\tV\tJ\tEpitope\n"
        b"CASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\tGIL\n"
        b"CASSIRSSYEQYF\tTRBV2*01\tTRBJ1*01\tNLV\n"
        b"CASSIRSS_EQYF\tTRBV1*01\tTRBJ1*01\tGLC\n"
        b"WWWSIRSSYEQWW\tTRBV1*01\tTRBJ1*01\tELA\n")


def test_the_stage_over_a_stubbed_native_call(tmp_path, monkeypatch, capsys):
    files, db = write_inputs(tmp_path, [("A", W_ROWS)], db=W_DB)
    calls = []
    mu.StubIndex.made.clear()
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_match_weighted", wu.brute_force_native(calls))
    monkeypatch.setattr(nat, "cdr3_match", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the weighted stage called cdr3_match")))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    res = mt.run(dict(command="match", infile=files, database=db, outpath=out, prefix="t_", dontgzip=True, cdr3_metric="weighted", **DB_FLAGS))
    head = b"clonotype\tv_call\tj_call\tjunction_aa\tduplicate_count\ttarget\tdistance\tdb_CDR3\tdb_V\tdb_J\tdb_Epitope\n"
    # I-L costs 6, W-L 12; one residue less is a gap of 12 at the best place; the trimmed ends of WWWSIRSSYEQWW do not count
    assert open(res["matches"][0], "rb").read() == head + (
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t0\t6\tCASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\tGIL\n"
        b"0\tTRBV1*01\tTRBJ1*01\tCASSIRSSYEQYF\t10\t3\t0\tWWWSIRSSYEQWW\tTRBV1*01\tTRBJ1*01\tELA\n"
        b"1\tTRBV1*01\tTRBJ1*01\tCASSWRSSYEQYF\t5\t0\t12\tCASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\tGIL\n"
        b"1\tTRBV1*01\tTRBJ1*01\tCASSWRSSYEQYF\t5\t3\t12\tWWWSIRSSYEQWW\tTRBV1*01\tTRBJ1*01\tELA\n"
        b"2\tTRBV1*01\tTRBJ1*01\tCASSIRSYEQYF\t3\t0\t18\tCASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\tGIL\n"
        b"2\tTRBV1*01\tTRBJ1*01\tCASSIRSYEQYF\t3\t3\t12\tWWWSIRSSYEQWW\tTRBV1*01\tTRBJ1*01\tELA\n"
        b"4\tTRBV2*01\tTRBJ1*01\tCASSIRSSYEQYF\t1\t1\t0\tCASSIRSSYEQYF\tTRBV2*01\tTRBJ1*01\tNLV\n")
    assert open(res["targets"], "rb").read() == (b"target\tdb_CDR3\tdb_V\tdb_J\tdb_Epitope\tA_clonotypes\tA_reads\n"
                                                 b"0\tCASSLRSSYEQYF\tTRBV1*01\tTRBJ1*01\tGIL\t3\t18\n"
                                                 b"1\tCASSIRSSYEQYF\tTRBV2*01\tTRBJ1*01\tNLV\t1\t1\n"
                                                 b"3\tWWWSIRSSYEQWW\tTRBV1*01\tTRBJ1*01\tELA\t3\t18\n")
    assert len(calls) == 1 and calls[0][5] == 24 and (calls[0][4].gap, calls[0][4].ntrim, calls[0][4].ctrim) == (12, 3, 2)
    assert len(mu.StubIndex.made) == 1 and mu.StubIndex.made[0].closed
    assert capsys.readouterr().out.splitlines()[0] == (
        "Match of A against 4 database entries (weighted, radius 24, gap 12, trim 3,2, class v): 6 clonotypes, 4 with a hit (19 reads), "
        "7 hits, 0 clonotypes and 0 entries out of reach, 2 clonotypes and 1 entries left out for a byte outside A..Z")
    assert mt.stats["A"]["queries_not_letters"] == 2 and mt.stats["A"]["targets_not_letters"] == 1
    # other settings reach the call: radius 6 keeps the conservative substitution and the free ends alone
    calls.clear()
    res = mt.run(dict(command="match", infile=files, database=db, outpath=out, prefix="u_", dontgzip=True, cdr3_metric="weighted",
                      cdr3_radius=6, cdr3_gap_cost=30, cdr3_trim="0,0", **DB_FLAGS))
    assert calls[0][5] == 6 and (calls[0][4].gap, calls[0][4].ntrim, calls[0][4].ctrim) == (30, 0, 0)
    assert [ln.split(b"\t")[5:7] for ln in open(res["matches"][0], "rb").read().splitlines()[1:]] == [[b"0", b"6"], [b"1", b"0"]]


def test_without_the_flag_the_stage_is_what_it_was(tmp_path, monkeypatch, capsys):
    files, db = write_inputs(tmp_path, [("A", A_ROWS)], db=DB)
    monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
    monkeypatch.setattr(nat, "cdr3_match", mu.brute_force_native())
    monkeypatch.setattr(nat, "cdr3_match_weighted", lambda *a, **k: (_ for _ in ()).throw(AssertionError("weighted without the flag")))
    out = str(tmp_path) + os.sep
    res = mt.run(dict(command="match", infile=files, database=db, outpath=out, prefix="t_", dontgzip=True, **DB_FLAGS))
    assert capsys.readouterr().out.splitlines()[0] == ("Match of A against 4 database entries (hamming 1, class v): 4 clonotypes, 2 with a hit "
                                                       "(11 reads), 3 hits, 0 clonotypes and 0 entries out of reach")
    assert set(res["stats"][0]) == set(nat.CDR3_MATCH_STATS)
