"""`match --cdr3-metric weighted` through the HIP path: dcrx_cdr3_match_weighted_run against the contract written in Python
(tests/cdr3_wmatch_util.py) — degree, the CSR of hits, every hit's distance, the targets' totals and the statistics, exactly,
and the distances against the host formatter's column — on the constructed lists (every length and position, gap positions,
sums past 2^12, the trims' limits, non-letters, tile and block edges, missing buckets, class bits), the primitive's work space
and hit rules, one index under all three metrics, one larger table, the unit-cost cross-check and the sub-command end to end."""
import ctypes as C
import gzip
import os
import time

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from tests import cdr3_match_util as mu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu

pytestmark = pytest.mark.gpu


def _column(case, result, cost):
    """The distance column of dcrx_format_cdr3_matches_weighted over a result's hits."""
    q_off, q_text = cnu.node_text(case.q_strings)
    t_off, t_text = cnu.node_text(case.t_strings)
    m = len(case.q_strings)
    text = nat.format_cdr3_matches_weighted(result, [0] * m, [0] * m, ["V"], ["J"], q_off, q_text, case.weights, t_off, t_text, b"db_x",
                                            [b"x"] * len(case.t_strings), cost)
    return [int(ln.split(b"\t")[6]) for ln in text.splitlines()[1:]]


def _check(case, cost, R, want=None, column=True):
    want = want or wu.expected(case, cost, R)
    got = wu.native_match(case, cost, R)
    wu.assert_same(got, want, R)
    if column:
        assert _column(case, got, cost) == got["hit_dist"].tolist()
    return want


def _names(*prefixes):
    return [n for n in wu.NAMES if n.startswith(prefixes)]


# ---- the constructed lists (each asserted its premise on the Python result when it was built) ----

@pytest.mark.parametrize("name", _names("equal_", "trimmed_", "conservative_", "no_"))
def test_no_node_and_one_node_a_side(name):
    _check(*wu.constructed()[name])


@pytest.mark.parametrize("L", wu.LENGTHS)
def test_a_substitution_at_every_position_in_both_directions(L):
    for longer in ("target", "query"):
        case, cost, R = wu.constructed()[f"length_{L}_{longer}_longer"]
        want = _check(case, cost, R)
        assert (want["stats"]["hits"] > 0) == (L <= 32)
        _check(case, wu.default_cost(12, 0, 0), 24)      # every position counted: the single substitutions and the deletions alone


@pytest.mark.parametrize("name", _names("gap_", "nothing_counted_"))
def test_gap_positions_ties_and_nothing_counted(name):
    case, cost, R = wu.constructed()[name]
    _check(case, cost, R)
    _check(case.swapped(), cost, R)


@pytest.mark.parametrize("name", _names("sums_", "trim_"))
def test_sums_past_2_12_and_the_trims_limits(name):
    case, cost, R = wu.constructed()[name]
    want = _check(case, cost, R)
    assert name != "sums_past_2_12" or max(want["hit_dist"].tolist()) == 8160


@pytest.mark.parametrize("name", _names("non_letters"))
def test_non_letters_in_full_buckets_and_on_tile_edges(name):
    case, cost, R = wu.constructed()[name]
    want = _check(case, cost, R)
    assert want["stats"]["hits"] > 1000


@pytest.mark.parametrize("name", _names("targets_", "queries_", "gaps_", "class_bits_"))
def test_tile_and_block_edges_missing_buckets_and_class_bits(name):
    case, cost, R = wu.constructed()[name]
    want = _check(case, cost, R)
    assert want["stats"]["hits"] > 0
    if name.startswith("gaps_"):
        _check(case.swapped(), cost, R)


# ---- the primitive ----

def _primitive(index, case, cost, R, work_bytes=None, hit_cap=None, pattern=0xA5, twice=False, dist=True):
    """dcrx_cdr3_match_weighted_device over buffers and a stream of the caller's: (degree, hit_off, the whole hit and distance
    buffers, need, cap)."""
    _, (qc, off, text, _) = mu.native_args(case)
    m = len(qc)
    d_cls, d_off = nat.DeviceBuffer.from_host(qc), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_hit_off, d_need = nat.DeviceBuffer(max(16, m * 4)), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3_match_weighted_work_bytes(m, len(text)) if work_bytes is None else work_bytes
    assert wb > m * 32 or work_bytes is not None
    d_work = nat.DeviceBuffer(max(256, wb))
    stream = C.c_void_p()
    nat.check(nat.lib().dcrx_stream_create(C.byref(stream)))
    try:
        nat.cdr3_match_weighted_device(index, m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_hit_off, None, None, 0, d_need, d_work, wb,
                                       stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
        need = int(d_need.to_host(np.uint64, 1)[0])
        cap = need if hit_cap is None else hit_cap(need)
        room = max(need, cap) + 64
        d_hit = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        d_dist = nat.DeviceBuffer.from_host(np.full(room * 4, pattern, np.uint8))
        for _ in range(2 if twice else 1):      # two calls in a row on the caller's stream
            nat.cdr3_match_weighted_device(index, m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_hit_off, d_hit, d_dist if dist else None,
                                           cap, d_need, d_work, wb, stream)
        nat.check(nat.lib().dcrx_stream_synchronize(stream))
    finally:
        nat.lib().dcrx_stream_destroy(stream)
    assert int(d_need.to_host(np.uint64, 1)[0]) == need
    return (d_deg.to_host(np.uint32, m), d_hit_off.to_host(np.uint64, m + 1), d_hit.to_host(np.uint32, room), d_dist.to_host(np.uint32, room),
            need, cap)


def test_primitive_work_space_and_hit_rules():
    case = mu.classed(*mu.random_case(700, 1500, 3, 1, seed=9, length=(12, 14)), "v")
    cost, R = wu.default_cost(), 24
    want = wu.expected_numpy(case, cost, R)
    t_args, (_, _, text, _) = mu.native_args(case)
    assert nat.cdr3_match_weighted_work_bytes(1 << 30, 0) == 0
    assert nat.cdr3_match_weighted_work_bytes(1500, 0) == nat.cdr3_match_work_bytes(1500, 0, "hamming") > 0
    index = nat.Cdr3Index(*t_args)
    try:
        assert index.info()["device_bytes"] >= 92 * 700
        with pytest.raises(nat.DcrxError, match="work space is smaller") as e:
            _primitive(index, case, cost, R, work_bytes=nat.cdr3_match_weighted_work_bytes(1500, len(text)) - 1)
        assert e.value.code == -1
        filler = 0xA5A5A5A5
        deg, hit_off, hit, hd, need, cap = _primitive(index, case, cost, R, twice=True)
        assert need == cap == want["stats"]["hits"] == int(hit_off[-1]) and need > 200
        assert np.array_equal(deg, want["degree"]) and np.array_equal(hit_off, want["hit_off"])
        assert np.array_equal(hit[:need], want["hit"]) and np.array_equal(hd[:need], want["hit_dist"])
        assert (hit[need:] == filler).all() and (hd[need:] == filler).all()
        # one short, and half the need: the same need, nothing behind the cap is touched, every slot in front of it is right
        for short in (lambda n: n - 1, lambda n: n // 2):
            deg2, hit_off2, hit2, hd2, need2, cap2 = _primitive(index, case, cost, R, hit_cap=short)
            assert need2 == need and cap2 == short(need) and np.array_equal(deg2, deg) and np.array_equal(hit_off2, hit_off)
            assert (hit2[cap2:] == filler).all() and (hd2[cap2:] == filler).all()
            assert np.array_equal(hit2[:cap2], want["hit"][:cap2]) and np.array_equal(hd2[:cap2], want["hit_dist"][:cap2])
        # no distance buffer: the hits alone
        _, _, hit3, hd3, _, _ = _primitive(index, case, cost, R, dist=False)
        assert np.array_equal(hit3[:need], want["hit"]) and (hd3 == filler).all()
    finally:
        index.close()


# ---- one index, three metrics ----

def test_one_index_under_hamming_levenshtein_and_weighted_in_three_orders():
    case = mu.classed(*mu.random_case(500, 800, 3, 2, seed=31), "vj")
    ref = mu.Reference(case)
    cost = wu.default_cost()
    wants = {("hamming", 2): ref.expected(2, "hamming"), ("levenshtein", 2): ref.expected(2, "levenshtein"),
             ("levenshtein", 1): ref.expected(1, "levenshtein"), ("weighted", 24): wu.expected_numpy(case, cost, 24),
             ("weighted", 12): wu.expected_numpy(case, cost, 12)}
    assert wants[("weighted", 24)]["stats"]["hits"] > wants[("weighted", 12)]["stats"]["hits"] > 0
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        runs = list(wants)
        for order in (runs, runs[::-1], runs[1::2] + runs[::2]):
            for metric, limit in order:
                if metric == "weighted":
                    wu.assert_same(nat.cdr3_match_weighted(index, *q_args, cost, limit), wants[(metric, limit)], (metric, limit))
                else:
                    mu.assert_same(nat.cdr3_match(index, *q_args, limit, metric), wants[(metric, limit)], (metric, limit))
        assert index.info()["device_bytes"] >= 92 * 500
    finally:
        index.close()


def test_the_weight_sum():
    big = (1 << 64) - 1
    weights = [big - 299 * 7] + [7] * 299                         # the sum is 2^64 - 1: accepted, and the targets carry it
    case = mu.Case([0, 0], ["CASSLGQAYEQYF", "CAWWWWWWWWWWF"], [0] * 300, ["CASSIGQAYEQYF"] * 300, weights)
    want = _check(case, wu.default_cost(), 24, column=False)
    assert want["t_queries"].tolist() == [300, 0] and [int(x) for x in want["t_weight"]] == [big, 0]
    assert set(want["hit_dist"].tolist()) == {6} and want["stats"]["queries_hit_weight"] == big
    case.weights[1] += 1                                          # exactly 2^64: refused, on the host
    with pytest.raises(nat.DcrxError, match="2\\^64") as e:
        wu.native_match(case, wu.default_cost(), 24)
    assert e.value.code == nat.E_UNSUPPORTED


# ---- one larger table ----

def test_larger_table_equals_the_numpy_form_of_the_contract():
    """20 000 queries against 2 000 targets in 60 classes at R = 24; the reference (the literal minimum over every p, as array
    operations) takes a few seconds on one CPU thread and is timed here."""
    case = mu.classed(*mu.random_case(2000, 20000, 12, 5, seed=77, pool=800), "vj")
    assert len(set(case.t_classes) | set(case.q_classes)) == 60
    cost = wu.default_cost()
    t0 = time.perf_counter()
    want = wu.expected_numpy(case, cost, 24)
    print(f"reference: {time.perf_counter() - t0:.1f} s")
    st = want["stats"]
    assert 1000 < st["queries_hit"] < st["queries"] and 100 < st["targets_hit"] < st["targets"]
    hits = [(i, int(j)) for i in range(len(case.q_strings)) for j in want["hit"][int(want["hit_off"][i]):int(want["hit_off"][i + 1])]]
    assert {0, 6, 9, 12, 24} <= set(want["hit_dist"].tolist())
    assert sum(len(case.q_strings[i]) != len(case.t_strings[j]) for i, j in hits) > 100      # gapped hits
    _check(case, cost, 24, want, column=False)


# ---- the unit-cost cross-check against the other two metrics ----

@pytest.mark.parametrize("D", [1, 2])
def test_unit_costs_lie_between_hamming_and_levenshtein(D):
    case = mu.classed(*mu.random_case(500, 1200, 3, 2, seed=51, pool=500), "v")
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        ham = nat.cdr3_match(index, *q_args, D, "hamming")
        lev = nat.cdr3_match(index, *q_args, D, "levenshtein")
        got = nat.cdr3_match_weighted(index, *q_args, wu.unit_cost(), D)
    finally:
        index.close()
    pairs = lambda r: {(i, int(j)) for i in range(len(case.q_strings)) for j in r["hit"][int(r["hit_off"][i]):int(r["hit_off"][i + 1])]}
    assert pairs(ham) <= pairs(got) <= pairs(lev) and len(pairs(ham)) > 100 and len(pairs(got)) > len(pairs(ham))
    wu.assert_same(got, wu.expected_numpy(case, wu.unit_cost(), D))


# ---- the sub-command, end to end ----

def _clonotypes_text(rows) -> bytes:
    lines = ["\t".join(nat.CLONOTYPE_COLUMNS)]
    for v, j, aa, dup in rows:
        lines.append("\t".join([v, j, aa, str(dup)] + ["0"] * (len(nat.CLONOTYPE_COLUMNS) - 4)))
    return ("\n".join(lines) + "\n").encode("latin-1")


@pytest.mark.parametrize("flags,settings,mode", [([], (24, 12, 3, 2), "v"),
                                                 (["--cdr3-radius", "30", "--cdr3-gap-cost", "9", "--cdr3-trim", "2,1"], (30, 9, 2, 1), "vj")])
def test_sub_command_byte_for_byte(flags, settings, mode, tmp_path, capsys):
    ts, tv, tj, qs, qv, qj = mu.random_case(400, 900, 4, 2, seed=41)
    qs[5], ts[7], qs[9], ts[11] = "A" * 33, "", "CASSlGQAYEQYF", "CASS*GQAYEQYF"      # out of reach, and non-letters, on either side
    half = len(qs) // 2
    samples = [("S1", list(zip(qv[:half], qj[:half], qs[:half], range(1, half + 1)))),
               ("S2", list(zip(qv[half:], qj[half:], qs[half:], range(3, 3 + len(qs) - half))))]
    db_header = [b"Epitope", b"CDR3", b"V", b"J"]
    db_lines = [b"\t".join([b"EPI%d" % (k % 9), t.encode("latin-1"), v.encode(), j.encode()]) for k, (t, v, j) in enumerate(zip(ts, tv, tj))]
    db = tmp_path / "known.tsv.gz"
    with gzip.open(db, "wb") as fh:
        fh.write(b"\t".join(db_header) + b"\n" + b"\n".join(db_lines) + b"\n")
    files = []
    for name, rows in samples:
        files.append(str(tmp_path / (name + ".clonotypes.tsv")))
        open(files[-1], "wb").write(_clonotypes_text(rows))
    out = str(tmp_path / "out") + os.sep
    os.makedirs(out)
    pipeline.main(["match", "-in", *files, "-db", str(db), "-op", out, "-pf", "m_", "-dz", "--cdr3-metric", "weighted", *flags,
                   "--cdr3-class", mode, "--db-cdr3-column", "CDR3", "--db-v-column", "V", "--db-j-column", "J"])
    assert sorted(os.listdir(out)) == ["m_S1.cdr3_matches.tsv", "m_S2.cdr3_matches.tsv", "m_match_targets.tsv"]
    R, gap, ntrim, ctrim = settings
    cost = wu.default_cost(gap, ntrim, ctrim)
    results = []
    all_v, all_j = tv + [r[0] for _, rows in samples for r in rows], tj + [r[1] for _, rows in samples for r in rows]
    classes = cnu.call_classes(all_v, all_j, mode)
    at = len(ts)
    for name, rows in samples:
        case = mu.Case(classes[:len(ts)], ts, classes[at:at + len(rows)], [r[2] for r in rows], [r[3] for r in rows])
        at += len(rows)
        want = wu.expected_numpy(case, cost, R)
        assert want["stats"]["hits"] > 0
        results.append(want)
        text = wu.matches_text([r[0] for r in rows], [r[1] for r in rows], case, want, db_header, db_lines, cost)
        assert open(out + f"m_{name}.cdr3_matches.tsv", "rb").read() == text, name
    assert open(out + "m_match_targets.tsv", "rb").read() == mu.targets_text(["S1", "S2"], db_header, db_lines, results)
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 2 and printed[0].startswith(f"Match of S1 against 400 database entries (weighted, radius {R}, gap {gap}, trim")
    assert printed[0].endswith("1 clonotypes and 1 entries out of reach, 1 clonotypes and 1 entries left out for a byte outside A..Z")
