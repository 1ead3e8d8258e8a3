"""The radius profile on the device (include/dcrx.h "profile, weighted"): both entries against the contract in Python
(tests/cdr3_profile_util.py) on every cell over the constructed lists of tests/cdr3_wmatch_util.py, the identity with the weighted
match's degrees, the bin boundaries, the counters' width, a histogram of stale size, the empty shapes, the work space and the
caller's stream, and the `metaclonotypes` sub-command end to end."""
import os
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import metaclonotypes as mc
from tests import cdr3_match_util as mu
from tests import cdr3_profile_util as pu
from tests import cdr3_wmatch_util as wu
from tests.test_cdr3_match import clonotypes_text
from tests.test_gpu_work_space import _Out, _guarded

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _ladders(R):
    """step 1 up to R or the 32nd rung; step 3; and, where R > 0, R in one step."""
    return [pu.ladder_for(R, 1), pu.ladder_for(R, 3)] + ([(R, 2)] if R > 0 else [])


# ---- both entries, every cell, over the constructed lists ----

@pytest.mark.parametrize("name", wu.NAMES)
def test_both_entries_against_the_contract(name):
    case, cost, R = wu.constructed()[name]
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        for step, bins in _ladders(R):
            want = pu.expected_profile(case, cost, step, bins)
            if step == 1 and R + 1 == bins:      # the premise: the whole ladder holds what the list holds within R
                assert want.sum(axis=1).tolist() == wu.expected(case, cost, R)["degree"].tolist()
            got = pu.native_profile(case, cost, step, bins, index)
            assert got["profile"].dtype == np.uint32 and np.array_equal(got["profile"], want), (name, step, bins, "host entry")
            assert got["stats"] == pu.expected_stats(case, want), (name, step, bins)
            assert np.array_equal(pu.device_profile(case, cost, step, bins, index), want), (name, step, bins, "device entry")
    finally:
        index.close()


@pytest.mark.parametrize("name", ["targets_257", "queries_513", "non_letters"])
def test_prefix_sums_are_the_weighted_match_degrees_at_every_radius(name):
    case, cost, R = wu.constructed()[name]
    step, bins = 2, R // 2 + 1
    t_args, q_args = mu.native_args(case)
    index = nat.Cdr3Index(*t_args)
    try:
        cum = np.cumsum(pu.native_profile(case, cost, step, bins, index)["profile"].astype(np.uint64), axis=1)
        assert cum[:, -1].sum() > 0
        for b in range(bins):
            degree = nat.cdr3_match_weighted(index, *q_args, cost, b * step)["degree"]
            assert np.array_equal(cum[:, b], degree.astype(np.uint64)), (name, b * step)
    finally:
        index.close()


# ---- bin boundaries ----

def test_a_pair_at_distance_3_under_steps_1_to_4():
    case, cost, _ = wu.constructed()["conservative_at_cost"]
    assert wu.dist(case.q_strings[0], case.t_strings[0], cost) == 3
    for step, b in ((1, 3), (2, 2), (3, 1), (4, 1)):
        want = [[int(k == b) for k in range(4)]]
        assert pu.expected_profile(case, cost, step, 4).tolist() == want
        assert pu.native_profile(case, cost, step, 4)["profile"].tolist() == want and pu.device_profile(case, cost, step, 4).tolist() == want


@pytest.mark.parametrize("step,bins", [(272, 31), (8159, 2), (65535, 2), (1, 1)])
def test_pairs_at_exactly_the_top_and_one_past_it(step, bins):
    case, cost, _ = wu.constructed()["sums_past_2_12"]      # query 0 meets both targets at exactly 8 160
    want = pu.expected_profile(case, cost, step, bins)
    top = {(272, 31): [0] * 30 + [2], (8159, 2): [0, 0], (65535, 2): [0, 2], (1, 1): [0]}[(step, bins)]
    assert want[0].tolist() == top and (bins == 1 or want.sum() > 0)
    assert np.array_equal(pu.native_profile(case, cost, step, bins)["profile"], want)
    assert np.array_equal(pu.device_profile(case, cost, step, bins), want)


# ---- the counters' width ----

def test_a_cell_past_2_16_and_as_many_rows_of_one():
    n, cost = 66000, wu.default_cost()
    one_many = mu.Case([3] * n, [b"CASSIRSSYEQYF"] * n, [3, 4], [b"CASSIRSSYEQYF", b"CASSIRSSYEQYF"])
    got = pu.native_profile(one_many, cost, 2, 25)["profile"]
    assert got.tolist() == [[n] + [0] * 24, [0] * 25] and n > 1 << 16
    assert pu.device_profile(one_many, cost, 2, 25).tolist() == got.tolist()
    many_one = one_many.swapped()
    got = pu.native_profile(many_one, cost, 2, 25)
    assert got["profile"].shape == (n, 25) and (got["profile"][:, 0] == 1).all() and not got["profile"][:, 1:].any()
    assert got["stats"]["cells_sum"] == n == got["stats"]["queries_nonzero"]
    assert np.array_equal(pu.device_profile(many_one, cost, 2, 25), got["profile"])


# ---- 32 bins, then 1 bin over the same stream and work space ----

def test_a_histogram_of_stale_size_cannot_pass():
    cost = wu.unit_cost()
    case = mu.Case([0, 0, 0], [b"A" * 31, b"C" * 31, b"A" * 30 + b"C"], [0, 0], [b"A" * 31, b"C" * 31])
    assert wu.dist(b"A" * 31, b"C" * 31, cost) == 31
    wide, narrow = pu.expected_profile(case, cost, 1, 32), pu.expected_profile(case, cost, 1, 1)
    assert wide[0].tolist() == [1, 1] + [0] * 29 + [1] and narrow.tolist() == [[1], [1]]      # bins 0 and 31 of one row
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        q = pu.DeviceQueries(case)
        work = nat.cdr3_profile_weighted_work_bytes(q.m, q.text_bytes, 32)
        d_work, stream = nat.DeviceBuffer(work), nat.Stream()
        d_wide, d_narrow = _Out(np.uint32, q.m * 32), _Out(np.uint32, q.m)
        nat.cdr3_profile_weighted_device(index, *q.args(), cost, 1, 32, d_wide, d_work, work, stream.ptr)
        nat.cdr3_profile_weighted_device(index, *q.args(), cost, 1, 1, d_narrow, d_work, work, stream.ptr)
        stream.synchronize()
        assert np.array_equal(d_wide.read().reshape(q.m, 32), wide) and np.array_equal(d_narrow.read().reshape(q.m, 1), narrow)
    finally:
        index.close()


# ---- empty shapes ----

def test_empty_shapes():
    cost = wu.default_cost()
    for name in ("no_nodes", "no_targets", "no_queries"):
        case, _, _ = wu.constructed()[name]
        want = pu.expected_profile(case, cost, 2, 25)
        got = pu.native_profile(case, cost, 2, 25)
        assert got["profile"].shape == want.shape == (len(case.q_strings), 25) and not got["profile"].any()
        assert pu.device_profile(case, cost, 2, 25).tolist() == want.tolist()
    only_queries = mu.Case([1, 1], [b"CASSFEQYF", b"CASSWEQYF"], [1, 2, 1], [b"CASSFEQYF", b"CASSFEQYF", b"CASSYEQYF"])      # class 2: the queries' alone
    want = pu.expected_profile(only_queries, cost, 2, 25)
    assert want[1].tolist() == [0] * 25 and want[0, 0] == 1 and want[0].sum() == 2 == want[2].sum()
    assert np.array_equal(pu.native_profile(only_queries, cost, 2, 25)["profile"], want)
    assert np.array_equal(pu.device_profile(only_queries, cost, 2, 25), want)


# ---- the work space, the profile buffer, the refusals ----

def _case(m_q: int) -> mu.Case:
    """300 targets in three classes (three lengths mixed) and m_q queries, each a target's string or one a few edits away."""
    rnd = random.Random(77 + m_q)
    targets = [mu.code(i)[:11 - i % 3] for i in range(300)]
    t_classes = [k % 3 for k in range(300)]
    picks = [rnd.randrange(300) for _ in range(m_q)]
    return mu.Case(t_classes, targets, [t_classes[j] if rnd.random() < 0.8 else 5 for j in picks],
                   [mu.code((j + rnd.choice((0, 1, 20, 21, 400))) % 8000)[:11 - rnd.randrange(3)] for j in picks])


def _profile_run(index, case, cost, step, bins):
    q = pu.DeviceQueries(case)

    def run(d_work, size):
        d_profile = _Out(np.uint32, q.m * bins)      # exactly m_q * bins dwords, 0xA5 all over, a 64-byte tail that stays
        nat.cdr3_profile_weighted_device(index, *q.args(), cost, step, bins, d_profile, d_work, size)
        nat.synchronize()
        return (d_profile.read(),)
    return run, nat.cdr3_profile_weighted_work_bytes(q.m, q.text_bytes, bins)


@pytest.mark.parametrize("m_q", [1, 257])
@pytest.mark.parametrize("step,bins", [(2, 25), (48, 2)])
def test_work_space_and_profile_buffer(m_q, step, bins):
    case, cost = _case(m_q), wu.default_cost()
    want = pu.expected_profile_numpy(case, cost, step, bins)
    assert m_q < 257 or (want.sum() > 200 and (want.sum(axis=0) > 0).sum() >= min(bins, 3))
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        def check(outputs):
            assert np.array_equal(outputs[0].reshape(m_q, bins), want)
        _guarded(*_profile_run(index, case, cost, step, bins), before=_profile_run(index, _case(1500), cost, 2, 32), check=check)
    finally:
        index.close()


def test_refusals_launch_nothing():
    case, cost = _case(5), wu.default_cost()
    index = nat.Cdr3Index(*mu.native_args(case)[0])
    try:
        q = pu.DeviceQueries(case)
        work = nat.cdr3_profile_weighted_work_bytes(q.m, q.text_bytes, 32)
        d_work = nat.DeviceBuffer(work + 256)
        d_profile = _Out(np.uint32, q.m * 32)
        asym = cost.sub.copy()
        asym[1, 3] = 5

        class Shifted:
            ptr = d_work.ptr + 64
        calls = [(nat.Cdr3Cost(asym), 2, 25, d_profile, d_work, work), (nat.Cdr3Cost.default(gap=0), 2, 25, d_profile, d_work, work),
                 (None, 2, 25, d_profile, d_work, work), (cost, 0, 25, d_profile, d_work, work), (cost, 2, 0, d_profile, d_work, work),
                 (cost, 2, 33, d_profile, d_work, work), (cost, 65535, 3, d_profile, d_work, work), (cost, 2, 25, None, d_work, work),
                 (cost, 2, 25, d_profile, d_work, work - 1), (cost, 2, 25, d_profile, Shifted, work)]
        for c, step, bins, prof, wk, size in calls:
            with pytest.raises(nat.DcrxError) as e:
                nat.cdr3_profile_weighted_device(index, *q.args(), c, step, bins, prof, wk, size)
            assert e.value.code == E_INVALID, (step, bins)
        nat.synchronize()
        assert len(d_profile.read(0)) == 0      # (every byte is still 0xA5)
        _, (qc, off, text, _) = mu.native_args(case)
        for c, step, bins in [x[:3] for x in calls[:7]]:
            with pytest.raises(nat.DcrxError) as e:
                nat.cdr3_profile_weighted(index, qc, off, text, c, step, bins)
            assert e.value.code == E_INVALID
    finally:
        index.close()


def test_two_calls_in_a_row_on_the_callers_stream():
    cost = wu.default_cost()
    a, b = _case(257), _case(300)
    index = nat.Cdr3Index(*mu.native_args(a)[0])      # (the two cases share their targets)
    try:
        assert a.t_strings == b.t_strings and a.t_classes == b.t_classes
        qa, qb = pu.DeviceQueries(a), pu.DeviceQueries(b)
        work = nat.cdr3_profile_weighted_work_bytes(qb.m, qb.text_bytes, 25)
        d_work, stream = nat.DeviceBuffer(work), nat.Stream()
        out_a, out_b = _Out(np.uint32, qa.m * 25), _Out(np.uint32, qb.m * 2)
        nat.cdr3_profile_weighted_device(index, *qa.args(), cost, 2, 25, out_a, d_work, work, stream.ptr)
        nat.cdr3_profile_weighted_device(index, *qb.args(), cost, 48, 2, out_b, d_work, work, stream.ptr)      # no synchronise between
        stream.synchronize()
        assert np.array_equal(out_a.read().reshape(qa.m, 25), pu.expected_profile_numpy(a, cost, 2, 25))
        assert np.array_equal(out_b.read().reshape(qb.m, 2), pu.expected_profile_numpy(b, cost, 48, 2))
    finally:
        index.close()


# ---- the sub-command, end to end ----

def _stub_profile(index, classes, off, text, cost, step, bins):
    from tests import cdr3_network_util as cnu
    case = mu.Case(index.classes, index.strings, classes, cnu.node_strings(off, text))
    profile = pu.expected_profile_numpy(case, cost, int(step), int(bins))
    return {"profile": profile, "stats": pu.expected_stats(case, profile)}


def _stub_match(index, classes, off, text, weights, cost, radius):
    from tests import cdr3_network_util as cnu
    return wu.expected_numpy(mu.Case(index.classes, index.strings, classes, cnu.node_strings(off, text), weights), cost, int(radius))


def test_the_sub_command_end_to_end(tmp_path, monkeypatch, capsys):
    """About 300 clonotypes against about 2 000 background CDR3s: the three files of the device run are, byte for byte, those of
    the same stage over the contract in numpy."""
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
    files = {}
    for how in ("device", "contract"):
        out = str(tmp_path / how) + os.sep
        os.makedirs(out)
        if how == "contract":
            monkeypatch.setattr(nat, "Cdr3Index", mu.StubIndex)
            monkeypatch.setattr(nat, "cdr3_profile_weighted", _stub_profile)
            monkeypatch.setattr(nat, "cdr3_match_weighted", _stub_match)
        res = mc.run(dict(command="metaclonotypes", infile=[a_path], background=bg_path, outpath=out, prefix="", dontgzip=True,
                          strip_alleles=True, max_background_rate="1/1000", write_radius_profile=True, write_metaclonotype_members=True))
        files[how] = [open(x, "rb").read() for x in res["metaclonotypes"] + res["profiles"] + res["members"]]
        st = dict(mc.stats["S"])
        assert len(files[how]) == 3 and st["clonotypes"] == 300 and st["not_letters"] > 0
        assert 0 < st["with_neighbours"] <= st["with_radius"] < st["take_part"] < 300 and st["background_take_part"] < 2000
    assert files["device"] == files["contract"]
    assert len(files["device"][0].splitlines()) == 1 + st["take_part"] and len(files["device"][2].splitlines()) > 10
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Meta-clonotypes of S ")]
    assert len(lines) == 2 and lines[0] == lines[1]
