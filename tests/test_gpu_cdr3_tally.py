"""The tally on the device (include/dcrx.h "tally, weighted"): both entries against the contract in Python
(tests/cdr3_tally_util.py) on every cell over the constructed lists of tests/cdr3_wmatch_util.py under three patterns of radii,
the identity with the weighted match, a bound read from the wrong slot or left over from the tile before, a bound below the
length window, the counters' width, a tile every wave skips, stale outputs and a recycled work space on the caller's stream, the
work space and the refusals, the empty shapes, and `metaclonotypes` -> `tabulate` end to end."""
import os
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import metaclonotypes as mc
from decombinator_amd import tabulate as tb
from tests import cdr3_match_util as mu
from tests import cdr3_tally_util as tu
from tests import cdr3_wmatch_util as wu
from tests.test_cdr3_match import clonotypes_text
from tests.test_gpu_work_space import _Out, _guarded

pytestmark = pytest.mark.gpu

E_INVALID = -1
FIELDS = ("t_count", "t_weight", "q_degree")


def _both(case, cost, radii, want, what, index=None):
    """Both entries on a case against `want`, every cell (and the host entry's statistics)."""
    own = index or nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        tu.assert_same(tu.native_tally(case, cost, radii, own), want, (what, "host entry"))
        tu.assert_same(tu.device_tally(case, cost, radii, own), want, (what, "device entry"))
    finally:
        if index is None:
            own.close()


# ---- 1. both entries, every cell, over the constructed lists ----

@pytest.mark.parametrize("name", wu.NAMES)
def test_both_entries_against_the_contract(name):
    case, cost, R = wu.constructed()[name]
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        for pattern in tu.PATTERNS:
            radii = tu.radii_for(pattern, R, len(case.t_strings))
            _both(case, cost, radii, tu.expected_tally(case, cost, radii), (name, pattern), index)
    finally:
        index.close()


# ---- 2. the identity with the weighted match ----

@pytest.mark.parametrize("name", ["targets_257", "queries_513", "non_letters"])
def test_one_radius_is_the_weighted_match_and_mixed_radii_filter_its_hits(name):
    case, cost, R = wu.constructed()[name]
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        match = nat.cdr3_match_weighted(index, *q_args, cost, R)
        assert match["stats"]["hits"] > 0
        got = nat.cdr3_tally_weighted(index, *q_args, cost, tu.radii_for("all_R", R, len(case.t_strings)))
        assert np.array_equal(got["t_count"], match["t_queries"]) and np.array_equal(got["t_weight"], match["t_weight"])
        assert np.array_equal(got["q_degree"], match["degree"])
        radii = tu.radii_for("graded", R, len(case.t_strings))
        keep = match["hit_dist"].astype(np.int64) <= radii.astype(np.int64)[match["hit"]]
        want = np.bincount(match["hit"][keep].astype(np.int64), minlength=len(case.t_strings)).astype(np.uint32)
        got = nat.cdr3_tally_weighted(index, *q_args, cost, radii)
        assert np.array_equal(got["t_count"], want) and 0 < want.sum() < match["stats"]["hits"]
    finally:
        index.close()


# ---- 3. a bound from the wrong slot, or left over from the tile before ----

def test_twins_of_radius_0_and_48_in_opposite_order_in_two_tiles():
    """Ranks 254 and 255 close the first tile, 256 and 257 open the second: four copies of one string in one class with radii
    0, 48 | 48, 0 (the other targets are far away with radius 0); queries at distance 0, 3 and 12 of the twins."""
    cost = wu.default_cost()
    twin, far = b"CASSIRSSYEQYF", b"CASSPPPPPEQYF"
    targets = [far] * 254 + [twin] * 4 + [far] * 42
    radii = np.zeros(300, np.uint32)
    radii[[255, 256]] = 48
    queries = [twin, b"CASSVRSSYEQYF", b"CASSWRSSYEQYF"] * 3
    case = mu.Case([2] * 300, targets, [2] * 9, queries, weights=[1, 10, 100] * 3)
    want = tu.expected_tally(case, cost, radii)
    assert want["t_count"][254:258].tolist() == [3, 9, 9, 3] and want["t_weight"][254:258].tolist() == [3, 333, 333, 3]
    assert want["q_degree"].tolist() == [4, 2, 2] * 3 and not want["t_count"][:254].any() and not want["t_count"][258:].any()
    _both(case, cost, radii, want, "twins")


# ---- 4. a bound below the length window ----

def test_a_target_one_residue_longer_at_gap_minus_1_and_at_gap():
    cost = wu.default_cost()
    q, t = b"CASSLAPGATNEKLF", b"CASSLAPGWATNEKLF"      # one residue put in: the rest costs nothing
    assert wu.dist(q, t, cost) == cost.gap == 12
    case = mu.Case([0, 0, 0], [t, t, t], [0], [q], weights=[7])
    radii = [cost.gap - 1, cost.gap, cost.gap + 1]
    want = tu.expected_tally(case, cost, radii)
    assert want["t_count"].tolist() == [0, 1, 1] and want["t_weight"].tolist() == [0, 7, 7] and want["q_degree"].tolist() == [2]
    _both(case, cost, radii, want, "the length window")


# ---- 5. width ----

def test_a_count_past_2_16_and_a_weight_that_needs_64_bits():
    n, cost = 66000, wu.default_cost()
    s = b"CASSIRSSYEQYF"
    many = mu.Case([3, 4], [s, s], [3] * n, [s] * n, weights=[1] * n)      # 258 blocks, four waves each, onto one cell
    got = tu.native_tally(many, cost, [0, 0])
    assert got["t_count"].tolist() == [n, 0] and got["t_weight"].tolist() == [n, 0] and n > 1 << 16 and (got["q_degree"] == 1).all()
    dev = tu.device_tally(many, cost, [0, 0])
    assert all(np.array_equal(dev[k], got[k]) for k in FIELDS)
    heavy = mu.Case([3], [s], [3, 3, 3, 3], [s, s, s, b"CASSWRSSYEQYF"], weights=[1 << 40, 1 << 40, 1 << 40, 5])
    want = tu.expected_tally(heavy, cost, [3])
    assert want["t_weight"].tolist() == [3 << 40] and want["t_count"].tolist() == [3]
    _both(heavy, cost, [3], want, "2^40")
    heavier = mu.Case([3], [s], [3, 3], [s, s], weights=[(1 << 63) - 1, 1 << 63])      # the sum is 2^64 - 1: the last one that fits
    _both(heavier, cost, [0], tu.expected_tally(heavier, cost, [0]), "2^64 - 1")


# ---- 6. tiles that every wave skips ----

def test_a_class_between_two_whose_tiles_every_wave_skips():
    cost = wu.default_cost()
    strings = [mu.code(i)[:11 - i % 3] for i in range(256)]
    case = mu.Case([1] * 256 + [5] * 256 + [9] * 256, strings * 3, [5] * 300, [mu.code(i)[:11 - i % 3] for i in range(300)])
    radii = tu.radii_for("graded", 24, 768)
    want = tu.expected_tally_numpy(case, cost, radii)
    assert not want["t_count"][:256].any() and not want["t_count"][512:].any() and not want["t_weight"][:256].any()
    assert (want["t_count"][256:512] > 0).sum() > 150 and want["stats"]["hits"] > 1000
    _both(case, cost, radii, want, "classes 1, 5, 9")
    # the other way round: one block holds a wave of class 1 and waves of class 9, so the tile of class 5 is staged between two
    # tiles that are hit, and every wave skips it: it flushes nothing and leaves nothing for the tile behind it
    around = mu.Case(case.t_classes, case.t_strings, [1] * 64 + [9] * 150, case.q_strings[:214])
    want = tu.expected_tally_numpy(around, cost, radii)
    assert not want["t_count"][256:512].any() and (want["t_count"][:256] > 0).sum() > 50 and (want["t_count"][512:] > 0).sum() > 100
    _both(around, cost, radii, want, "classes 1 and 9 around 5")


# ---- 7. stale outputs, and one work space for two calls on the caller's stream ----

def _case(m_q: int) -> mu.Case:
    """300 targets in three classes (three lengths mixed) and m_q queries, each a target's string or one a few edits away."""
    rnd = random.Random(77 + m_q)
    targets = [mu.code(i)[:11 - i % 3] for i in range(300)]
    t_classes = [k % 3 for k in range(300)]
    picks = [rnd.randrange(300) for _ in range(m_q)]
    return mu.Case(t_classes, targets, [t_classes[j] if rnd.random() < 0.8 else 5 for j in picks],
                   [mu.code((j + rnd.choice((0, 1, 20, 21, 400))) % 8000)[:11 - rnd.randrange(3)] for j in picks])


def _outs(q, m_t):
    return _Out(np.uint32, m_t), _Out(np.uint64, m_t), _Out(np.uint32, q.m)


def test_two_calls_in_a_row_through_one_work_space_on_the_callers_stream():
    cost = wu.default_cost()
    a, b = _case(1500), _case(5)      # a large one, then a small one: the accumulators are zeroed per call
    ra, rb = tu.radii_for("graded", 48, 300), tu.radii_for("every_third_none", 12, 300)
    index = nat.Cdr3Index(*mu.native_args(a)[0])      # (the two cases share their targets)
    try:
        assert a.t_strings == b.t_strings and a.t_classes == b.t_classes
        qa, qb = tu.DeviceQueries(a), tu.DeviceQueries(b)
        work = nat.cdr3_tally_weighted_work_bytes(qa.m, qa.text_bytes, 300)
        assert work >= nat.cdr3_tally_weighted_work_bytes(qb.m, qb.text_bytes, 300)
        d_work, stream = nat.DeviceBuffer(work), nat.Stream()
        d_ra, d_rb = tu.device_radii(ra), tu.device_radii(rb)
        out_a, out_b = _outs(qa, 300), _outs(qb, 300)      # (0xA5 all over: every cell is written)
        nat.cdr3_tally_weighted_device(index, *qa.args(), cost, d_ra, *out_a, d_work, work, stream.ptr)
        nat.cdr3_tally_weighted_device(index, *qb.args(), cost, d_rb, *out_b, d_work, work, stream.ptr)      # no synchronise between
        stream.synchronize()
        want_a, want_b = tu.expected_tally_numpy(a, cost, ra), tu.expected_tally_numpy(b, cost, rb)
        assert want_a["stats"]["hits"] > 1000 and 0 < want_b["stats"]["hits"] < 100
        tu.assert_same(dict(zip(FIELDS, (o.read() for o in out_a))), {k: want_a[k] for k in FIELDS}, "the large call")
        tu.assert_same(dict(zip(FIELDS, (o.read() for o in out_b))), {k: want_b[k] for k in FIELDS}, "the small call behind it")
    finally:
        index.close()


# ---- 8. the work space, the outputs, the refusals ----

def _tally_run(index, case, cost, radii):
    q, m_t = tu.DeviceQueries(case), len(case.t_strings)
    d_r = tu.device_radii(radii)

    def run(d_work, size):
        outs = _outs(q, m_t)      # exactly the header's sizes, 0xA5 all over, a 64-byte tail that stays
        nat.cdr3_tally_weighted_device(index, *q.args(), cost, d_r, *outs, d_work, size)
        nat.synchronize()
        return tuple(o.read() for o in outs)
    return run, nat.cdr3_tally_weighted_work_bytes(q.m, q.text_bytes, m_t)


@pytest.mark.parametrize("m_q", [1, 257])
def test_work_space_and_outputs(m_q):
    case, cost = _case(m_q), wu.default_cost()
    radii = tu.radii_for("graded", 48, 300)
    want = tu.expected_tally_numpy(case, cost, radii)
    assert m_q < 257 or (want["stats"]["hits"] > 200 and want["stats"]["targets_hit"] > 50)
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        def check(outputs):
            tu.assert_same(dict(zip(FIELDS, outputs)), {k: want[k] for k in FIELDS})
        _guarded(*_tally_run(index, case, cost, radii), before=_tally_run(index, _case(1500), cost, tu.radii_for("all_R", 48, 300)), check=check)
    finally:
        index.close()


@pytest.mark.parametrize("m_q", [1, 257])
def test_refusals_launch_nothing(m_q):
    case, cost = _case(m_q), wu.default_cost()
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        q = tu.DeviceQueries(case)
        work = nat.cdr3_tally_weighted_work_bytes(q.m, q.text_bytes, 300)
        d_work, d_r = nat.DeviceBuffer(work + 256), tu.device_radii(tu.radii_for("all_R", 24, 300))
        tc, tw, deg = _outs(q, 300)
        asym = cost.sub.copy()
        asym[1, 3] = 5

        class Shifted:
            ptr = d_work.ptr + 64
        calls = [(nat.Cdr3Cost(asym), tc, tw, deg, d_work, work), (nat.Cdr3Cost.default(gap=0), tc, tw, deg, d_work, work),
                 (nat.Cdr3Cost.default(ntrim=17), tc, tw, deg, d_work, work), (None, tc, tw, deg, d_work, work),
                 (cost, None, tw, deg, d_work, work), (cost, tc, None, deg, d_work, work), (cost, tc, tw, None, d_work, work),
                 (cost, tc, tw, deg, d_work, work - 1), (cost, tc, tw, deg, Shifted, work), (cost, tc, tw, deg, None, work)]
        for c, a, b, d, wk, size in calls:
            with pytest.raises(nat.DcrxError) as e:
                nat.cdr3_tally_weighted_device(index, *q.args(), c, d_r, a, b, d, wk, size)
            assert e.value.code == E_INVALID
        nat.synchronize()
        assert all(len(o.read(0)) == 0 for o in (tc, tw, deg))      # (every byte is still 0xA5)
        _, q_args = mu.native_args(case)
        for c in [x[0] for x in calls[:4]]:
            with pytest.raises(nat.DcrxError) as e:
                nat.cdr3_tally_weighted(index, *q_args, c, tu.radii_for("all_R", 24, 300))
            assert e.value.code == E_INVALID
        for bad in (65536, 0xFFFFFFFE):      # the host entry sees the radii
            radii = tu.radii_for("every_third_none", 24, 300)
            radii[299] = bad
            assert tu.host_refuses(radii)
            with pytest.raises(nat.DcrxError, match="a radius is 0 .. 65535") as e:
                nat.cdr3_tally_weighted(index, *q_args, cost, radii)
            assert e.value.code == E_INVALID
    finally:
        index.close()


def test_the_device_entry_takes_a_value_above_65535_for_no_radius():
    case, cost, R = wu.constructed()["targets_257"]
    radii = tu.radii_for("all_R", R, len(case.t_strings))
    radii[::2] = 65536
    radii[1] = 0xFFFFFFFE
    want = tu.expected_tally(case, cost, radii)
    assert not want["t_count"][::2].any() and want["t_count"].any()
    tu.assert_same(tu.device_tally(case, cost, radii), {k: want[k] for k in FIELDS})


# ---- 9. empty shapes ----

def test_empty_shapes():
    cost = wu.default_cost()
    for name in ("no_nodes", "no_targets", "no_queries"):
        case, _, _ = wu.constructed()[name]
        radii = tu.radii_for("all_R", 24, len(case.t_strings))
        want = tu.expected_tally(case, cost, radii)
        assert want["stats"]["hits"] == 0
        _both(case, cost, radii, want, name)      # (the outputs come filled with 0xA5: no queries zero the targets' cells, and the other way)
    only_queries = mu.Case([1, 1], [b"CASSFEQYF", b"CASSWEQYF"], [1, 2, 1], [b"CASSFEQYF", b"CASSFEQYF", b"CASSYEQYF"])      # class 2: the queries' alone
    want = tu.expected_tally(only_queries, cost, [24, 24])
    assert want["q_degree"].tolist() == [2, 0, 2] and want["t_count"].tolist() == [2, 2]
    _both(only_queries, cost, [24, 24], want, "a class the queries alone hold")
    none = [tu.NO_RADIUS, tu.NO_RADIUS]
    want = tu.expected_tally(only_queries, cost, none)
    assert want["stats"]["hits"] == 0 and want["stats"]["targets_without_radius"] == 2
    _both(only_queries, cost, none, want, "no target has a radius")


# ---- 10. metaclonotypes -> tabulate, end to end ----

def test_the_round_trip_end_to_end(tmp_path, monkeypatch, capsys):
    """About 300 clonotypes against about 2 000 background CDR3s through `metaclonotypes`, then `tabulate -mc` on its own output
    with the same sample: every row with a radius holds sample_neighbours + 1 clonotypes (the neighbours and itself), and the
    two files of the device run are, byte for byte, those of the same stage over the contract in numpy."""
    rnd = random.Random(5)
    vs = [f"TRBV{k}*0{1 + k % 2}" for k in range(1, 7)]
    string = lambda i: (mu.code(i)[:11 - i % 3] if i % 97 else "CASS*" + mu.code(i)[5:])
    bg = ["junction_aa\tv_call\tj_call"] + [f"{string(rnd.randrange(1000))}\t{rnd.choice(vs)}\tTRBJ1-1*01" for _ in range(2000)]
    rows = [(rnd.choice(vs), "TRBJ1-1*01", string(rnd.randrange(400)), 1 + rnd.randrange(50)) for _ in range(300)]
    bg_path, a_path = str(tmp_path / "bg.tsv"), str(tmp_path / "S.clonotypes.tsv")
    with open(bg_path, "w") as fh:
        fh.write("\n".join(bg) + "\n")
    with open(a_path, "wb") as fh:
        fh.write(clonotypes_text(rows))
    first = str(tmp_path / "mc") + os.sep
    os.makedirs(first)
    res = mc.run(dict(command="metaclonotypes", infile=[a_path], background=bg_path, outpath=first, prefix="", dontgzip=True,
                      strip_alleles=True, max_background_rate="1/1000"))
    mc_path = res["metaclonotypes"][0]
    files = {}
    for how in ("device", "contract"):
        out = str(tmp_path / how) + os.sep
        os.makedirs(out)
        if how == "contract":
            monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
            monkeypatch.setattr(nat, "cdr3_tally_weighted", tu.brute_force_native(numpy_form=True))
        got = tb.run(dict(command="tabulate", infile=[a_path], metaclonotypes=mc_path, outpath=out, prefix="", dontgzip=True, strip_alleles=True))
        files[how] = [open(got[k], "rb").read() for k in ("tabulate", "samples")]
    assert files["device"] == files["contract"]
    made = [x.split(b"\t") for x in open(mc_path, "rb").read().splitlines()[1:]]
    table = [x.split(b"\t") for x in files["device"][0].splitlines()]
    assert table[0][:6] == [b"metaclonotype", b"v_call", b"j_call", b"junction_aa", b"radius", b"samples"] and table[0][6:] == [b"S_clonotypes", b"S_reads"]
    with_radius = [(k, f) for k, f in enumerate(made) if f[5] != b"."]
    assert 100 < len(with_radius) < len(made) and len(table) == 1 + len(with_radius)
    dup = {str(i).encode(): d for i, (_, _, _, d) in enumerate(rows)}
    some = 0
    for (k, f), line in zip(with_radius, table[1:]):
        assert line[0] == str(k).encode() and line[1:5] == [f[1], f[2], f[3], f[5]]
        assert int(line[6]) == int(f[8]) + 1 and int(line[5]) == 1 and int(line[7]) >= dup[f[0]]      # the neighbours, and itself
        some += int(f[8]) > 0
    assert some > 10
    st = tb.stats["S"]
    assert st["clonotypes"] == 300 and len(with_radius) <= st["clonotypes_inside"] <= st["take_part"] < 300 and 0 < st["reads_inside"] <= st["reads"]
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Tabulated S ")]
    assert len(lines) == 2 and lines[0] == lines[1]
