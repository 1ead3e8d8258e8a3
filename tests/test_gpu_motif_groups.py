"""`motifs --groups` through the HIP path: dcrx_cdr3_motif_members_device, dcrx_cdr3_groups_device and dcrx_cdr3_motif_groups
against the contract written in Python (gu.expected_groups: sets of slices, every pair of units compared, a union-find in a
dict) — every field, `need` and the statistics exactly — on tables around a block of units, a unit with 90 postings, rows of
members around a wave and over several blocks, many rows of one member, units that take no part, no selected motif (the
network's clusters), no distance, an alternating chain of 40 links, `cap` at 0, below and at `need`, work spaces one byte short
and misaligned, selected motifs the host entry refuses, a stream of the caller's, one random table, and the sub-command end to
end.  Every refusal here is decided on the host before any launch."""
import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import motifs, pipeline
from decombinator_amd.match import spans
from tests import motif_groups_util as gu
from tests import motif_util as mu
from tests import test_motif_groups as cpu

pytestmark = pytest.mark.gpu

E_INVALID = -1
FILL = b"GHIKLMNPQRST"      # letters of which no motif below is made


def _check(units, selected, ks=(2, 3, 4), trim=(3, 3), G=1, weights=None):
    units = [bytes(u) for u in units]
    weights = list(range(1, len(units) + 1)) if weights is None else weights
    off, text = spans(units)
    got = nat.cdr3_motif_groups(off, text, weights, ks, trim, [k for k, _ in selected], [c for _, c in selected], G)
    want = gu.expected_groups(units, weights, ks, trim, selected, G)
    gu.assert_same(got, want)
    return got, want


def ints(a):
    return [int(x) for x in a]


def _pool():
    return mu.random_units(400, 21, 8, 14)


_motifs_held_twice = gu.motifs_held


def _mutants(units, seed):
    """Every unit with one residue replaced (so that it has a neighbour), the position and the letter seeded."""
    rng = np.random.default_rng(seed)
    out = []
    for u in units:
        p = int(rng.integers(0, len(u)))
        out.append(u[:p] + bytes([mu.AMINO[(mu.AMINO.index(u[p]) + 1 + int(rng.integers(0, 19))) % 20]]) + u[p + 1:])
    return out


def _tagged(motif: bytes, i: int) -> bytes:
    """A unit that holds `motif` right behind the trim and no other motif made of its letters: the tail spells i."""
    return b"XXX" + motif + bytes([FILL[i // 144 % 12], FILL[i // 12 % 12], FILL[i % 12]]) + b"XXX"


# ---- units around a block ----

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_units_around_a_block(n):
    units = list(_pool()[:n])
    selected = _motifs_held_twice(units, (2, 3), (3, 3)) if n > 1 else cpu.sel("AC", "CAS")
    got, _ = _check(units, selected, ks=(2, 3))
    assert got["stats"]["groups"] <= n and (n < 255 or got["need"] > n)


def test_one_unit_of_32_letters_with_90_postings_and_a_twin():
    unit = bytes(mu.AMINO) + b"ADFHKMPRTWBJ"      # no two-letter window twice: 31 + 30 + 29 motifs
    held = sorted(mu.motif_set(unit, (2, 3, 4), (0, 0)))
    assert len(unit) == 32 and len(held) == 90
    selected = [(k, mu.code_of(w)) for k, w in held]
    got, _ = _check([unit], selected, trim=(0, 0))
    assert got["need"] == 90 and ints(got["n_motifs"]) == [90] and ints(got["mem"]) == [0] * 90
    got, _ = _check([b"CASSF", unit, unit[:31] + b"A", unit], selected, trim=(0, 0))      # (the twins are linked by every row)
    assert ints(got["n_motifs"])[1] == 90 == ints(got["n_motifs"])[3] and ints(got["group_of"])[1] == ints(got["group_of"])[3]


def test_a_unit_of_one_letter_holds_each_motif_once():
    got, _ = _check([b"AAAAAAAA", b"AAAAAAAC"], cpu.sel("AA", "AAA", "AAAA"), trim=(0, 0), G=0)
    assert ints(got["n_motifs"]) == [3, 3] and ints(got["mem"]) == [0, 1] * 3 and got["need"] == 6


# ---- the rows' postings ----

def test_rows_of_63_64_65_and_600_members():
    """The postings lie row after row: AA's fill lanes 0 .. 62 of the first wave, CC's first is its last lane and CC's next begins
    the second wave in lane 0; EE's 600 run over several blocks.  The units come shuffled, so a row's smallest label is anywhere
    in it; without the distance only the rows join anything: four groups."""
    units = [_tagged(m, i) for m, count in ((b"AA", 63), (b"CC", 64), (b"DD", 65), (b"EE", 600)) for i in range(count)]
    order = np.random.default_rng(4).permutation(len(units))
    units = [units[int(i)] for i in order]
    got, _ = _check(units, cpu.sel("AA", "CC", "DD", "EE"), ks=(2,), G=0)
    assert ints(got["mem_off"]) == [0, 63, 127, 192, 792] and sorted(ints(got["units"])) == [63, 64, 65, 600]
    assert got["stats"]["groups"] == 4 and got["stats"]["mixed_groups"] == 0 and got["stats"]["rounds"] >= 2
    _check(units, cpu.sel("AA", "CC", "DD", "EE"), ks=(2,), G=1)


def test_many_rows_of_one_member_each():
    letters = mu.AMINO
    units = [b"XXX" + bytes([letters[i // 400 % 20], letters[i // 20 % 20], letters[i % 20], letters[(7 * i) % 20]]) + b"XXX" for i in range(900)]
    selected = sorted(((4, mu.code_of(u[3:7])) for u in units), key=lambda kc: kc[1])
    got, _ = _check(units, selected, ks=(4,), G=0)
    assert got["need"] == 900 and got["stats"]["groups"] == 900 == got["stats"]["singleton_groups"]
    assert ints(np.diff(got["mem_off"].astype(np.int64))) == [1] * 900


# ---- units that take no part; no selected motif; no distance ----

def test_units_that_take_no_part_are_groups_of_their_own_unless_the_distance_links_them():
    units = [b"", b"A" * 33, b"CASSLG*EF", b"CASSLGsEF", b"CASSLGYEF", b"CASSLGYEW", b"CASSLGWEF", b"\x00\xffAB", b"CASS"]
    got, want = _check(units, cpu.sel("SL", "LG", "SLG"), G=1)
    assert ints(got["n_motifs"])[:4] == [0, 0, 0, 0] and got["stats"]["take_part"] == 4
    # the unit with `*` and the lower-case one are one residue from CASSLGYEF and from each other: linked, exactly as the
    # network links them when every class is equal
    off, text = spans(units)
    net, _ = nat.cdr3_network(np.zeros(len(units), np.uint32), off, text, np.ones(len(units), np.uint64), 1)
    assert ints(got["degree"]) == ints(net["degree"]) and ints(got["degree"])[2] == 3 and ints(got["degree"])[:2] == [0, 0]
    assert ints(got["group_of"])[2] == ints(got["group_of"])[4] and ints(got["units"])[ints(got["group_of"])[0]] == 1
    alone, _ = _check(units, cpu.sel("SL", "LG", "SLG"), G=0)
    assert ints(alone["units"])[ints(alone["group_of"])[2]] == 1 and ints(alone["degree"]) == [0] * len(units)


@pytest.mark.parametrize("G", [1, 2])
def test_without_a_selected_motif_the_groups_are_the_networks_clusters(G):
    base = list(_pool()[:300])
    units = list(dict.fromkeys(base + _mutants(base[:150], 9) + _mutants(base[100:200], 10)))
    weights = [3 * i + 1 for i in range(len(units))]
    got, _ = _check(units, [], G=G, weights=weights)
    off, text = spans(units)
    net, st = nat.cdr3_network(np.zeros(len(units), np.uint32), off, text, np.array(weights, np.uint64), G)
    for mine, theirs in (("group_of", "cluster_of"), ("head", "cluster_head"), ("units", "cluster_size"), ("weight", "cluster_weight"),
                         ("degree", "degree")):
        assert ints(got[mine]) == ints(net[theirs]), mine
    assert got["stats"]["global_edges"] == st["edges"] > 100 and got["stats"]["groups"] == st["clusters_out"] and got["need"] == 0


def test_without_the_distance_only_the_motifs_join():
    units = list(_pool()[:200]) + _mutants(_pool()[:50], 3)
    selected = _motifs_held_twice(units, (3, 4), (3, 3))
    got, _ = _check(units, selected, ks=(3, 4), G=0)
    assert got["stats"]["global_edges"] == 0 and 1 < got["stats"]["groups"] < len(units) and len(selected) > 10


# ---- the rounds ----

def _chain():
    """41 units in a chain of 40 links, motif row and one-residue link in turn: a_t and b_t hold YZ<z_t> (and nobody else does);
    b_t and a_(t+1) differ in that one letter alone (and have a flank nobody else has).  The lowest index sits at the far end,
    the others are shuffled: (units by index, the chain's indices from end to end)."""
    z = [bytes([65 + t]) for t in range(21)]
    chain = []
    for t in range(21):
        if t:
            chain.append(bytes([65 + t - 1]) * 3 + b"YZ" + z[t] + b"W" + b"GGG")      # a_t: b_(t-1)'s flank
        else:
            chain.append(b"ZZZ" + b"YZ" + z[0] + b"W" + b"GGG")
        if t < 20:
            chain.append(bytes([65 + t]) * 3 + b"YZ" + z[t] + b"W" + b"GGG")          # b_t
    assert len(chain) == 41
    index = [int(i) + 1 for i in np.random.default_rng(2).permutation(40)] + [0]
    units = [None] * 41
    for p, i in enumerate(index):
        units[i] = chain[p]
    return units, index


def test_an_alternating_chain_of_40_links_is_one_group():
    units, index = _chain()
    selected = sorted(((3, mu.code_of(b"YZ" + bytes([65 + t]))) for t in range(21)), key=lambda kc: kc[1])
    # a label has to pass row, link, row, ...: position p is joined to p + 1 by a row (p even) or by the distance (p odd) alone
    want = gu.expected_groups(units, [1] * 41, (3,), (3, 3), selected, 1)
    assert ints(np.diff(want["mem_off"].astype(np.int64))) == [2] * 20 + [1] and want["stats"]["global_edges"] == 20
    assert sum(d == 1 for d in ints(want["degree"])) == 40 and max(ints(want["degree"])) == 1
    # more than one unit is smaller than both its neighbours: the first round cannot carry index 0 to everyone, so the rows,
    # the units and the jumps work over several rounds (a round more sees nothing move)
    minima = [p for p in range(41) if all(index[p] < index[q] for q in (p - 1, p + 1) if 0 <= q <= 40)]
    assert len(minima) > 3
    got, _ = _check(units, selected, ks=(3,), G=1, weights=[1] * 41)
    assert ints(got["group_of"]) == [0] * 41 and ints(got["units"]) == [41] and got["stats"]["mixed_groups"] == 1
    assert got["stats"]["rounds"] >= 3
    halves, _ = _check(units, selected, ks=(3,), G=0, weights=[1] * 41)
    assert halves["stats"]["groups"] == 21 and halves["stats"]["largest_group"] == 2


# ---- the members primitive: cap, work space, stream ----

def _members_case():
    units = list(_pool()[:120])
    return units, _motifs_held_twice(units, (2, 3), (3, 3))


def test_members_cap_0_below_need_and_at_need():
    units, selected = _members_case()
    off, text = spans(units)
    whole = gu.expected_members(units, (2, 3), (3, 3), selected)
    need = whole["need"]
    assert need > 300
    for cap in (0, 1, need - 1, need, need + 5, None):
        got = nat.cdr3_motif_members(off, text, (2, 3), (3, 3), [k for k, _ in selected], [c for _, c in selected], cap)
        gu.assert_same_members(got, gu.expected_members(units, (2, 3), (3, 3), selected, cap))
        assert got["need"] == need and len(got["mem"]) == (need if cap is None else min(cap, need))


class _At:
    """A device address inside a DeviceBuffer."""

    def __init__(self, buf, shift):
        self.ptr = buf.ptr + shift


def _members_buffers(units, selected, cap):
    off, text = spans(units)
    n, S = len(units), len(selected)
    work = nat.cdr3_motif_members_work_bytes(n, cap)
    assert work > 0
    return {"n": n, "S": S, "cap": cap, "work_bytes": work, "work": nat.DeviceBuffer(work + 256),
            "in": [nat.DeviceBuffer.from_host(np.asarray(off, np.uint64)), nat.DeviceBuffer.from_host(np.frombuffer(text, np.uint8)),
                   nat.DeviceBuffer.from_host(np.array([k for k, _ in selected], np.uint32)),
                   nat.DeviceBuffer.from_host(np.array([c for _, c in selected], np.uint32))],
            "out": [nat.DeviceBuffer(4 * n), nat.DeviceBuffer(8 * (S + 1)), nat.DeviceBuffer(4 * cap + 16), nat.DeviceBuffer(16)]}


def _members_call(b, ks, trim, stream=None, short=0, shift=0):
    i, o = b["in"], b["out"]
    nat.cdr3_motif_members_device(b["n"], i[0], i[1], ks, trim, b["S"], i[2], i[3], b["cap"], o[0], o[1], o[2], o[3], _At(b["work"], shift),
                                  b["work_bytes"] - short, None if stream is None else stream.ptr)


def _members_result(b):
    need = int(b["out"][3].to_host(np.uint64, 1)[0])
    return {"n_motifs": b["out"][0].to_host(np.uint32, b["n"]), "mem_off": b["out"][1].to_host(np.uint64, b["S"] + 1),
            "mem": b["out"][2].to_host(np.uint32, min(need, b["cap"])), "need": need}


def test_members_twice_on_a_stream_of_the_callers():
    units, selected = _members_case()
    need = gu.expected_members(units, (2, 3), (3, 3), selected)["need"]
    b = _members_buffers(units, selected, need)
    stream = nat.Stream()
    _members_call(b, (2, 3), (3, 3), stream)
    _members_call(b, (2, 3), (3, 3), stream)      # into the same arrays and the same work space, nothing waited for between
    stream.synchronize()
    gu.assert_same_members(_members_result(b), gu.expected_members(units, (2, 3), (3, 3), selected))


def test_members_work_space_short_or_misaligned_is_refused_not_launched():
    units, selected = _members_case()
    need = gu.expected_members(units, (2, 3), (3, 3), selected)["need"]
    b = _members_buffers(units, selected, need)
    nat.check(nat.lib().dcrx_memset_device(b["out"][3].ptr, 0xAB, 8))
    for kwargs in ({"short": 1}, {"shift": 8}, {"shift": 128}):
        with pytest.raises(nat.DcrxError) as e:
            _members_call(b, (2, 3), (3, 3), **kwargs)
        assert e.value.code == E_INVALID
    nat.synchronize()
    assert int(b["out"][3].to_host(np.uint64, 1)[0]) == 0xABABABABABABABAB      # nothing ran
    _members_call(b, (2, 3), (3, 3), shift=256)
    nat.synchronize()
    gu.assert_same_members(_members_result(b), gu.expected_members(units, (2, 3), (3, 3), selected))


# ---- the groups primitive ----

_csr = gu.csr


def _groups_buffers(n, weights, adjacency, rows):
    adj_off, adj = _csr(adjacency)
    mem_off, mem = _csr(rows)
    S = len(rows)
    work = nat.cdr3_groups_work_bytes(n, S)
    assert work > 0
    return {"n": n, "S": S, "adj_entries": len(adj), "mem_entries": len(mem), "work_bytes": work, "work": nat.DeviceBuffer(work + 256),
            "in": [nat.DeviceBuffer.from_host(np.array(weights, np.uint64)), nat.DeviceBuffer.from_host(adj_off),
                   nat.DeviceBuffer.from_host(adj) if len(adj) else None, nat.DeviceBuffer.from_host(mem_off) if S else None,
                   nat.DeviceBuffer.from_host(mem) if len(mem) else None],
            "out": [nat.DeviceBuffer(4 * n + 16), nat.DeviceBuffer(4 * n + 16), nat.DeviceBuffer(4 * n + 16), nat.DeviceBuffer(8 * n + 16),
                    nat.DeviceBuffer(16)]}


def _groups_call(b, stream=None, short=0, shift=0):
    i, o = b["in"], b["out"]
    return nat.cdr3_groups_device(b["n"], i[0], i[1], i[2], b["adj_entries"], b["S"], i[3], i[4], b["mem_entries"], o[0], o[1], o[2], o[3],
                                  o[4], _At(b["work"], shift), b["work_bytes"] - short, None if stream is None else stream.ptr)


def _groups_result(b):
    g = int(b["out"][4].to_host(np.uint32, 1)[0])
    return {"group_of": b["out"][0].to_host(np.uint32, b["n"]), "head": b["out"][1].to_host(np.uint32, g),
            "units": b["out"][2].to_host(np.uint32, g), "weight": b["out"][3].to_host(np.uint64, g)}


def _groups_case():
    """An adjacency that is no Hamming one (a ring over every seventh unit) beside the rows of a real table."""
    units = list(_pool()[:300])
    n = len(units)
    rows = gu.expected_members(units, (3,), (3, 3), _motifs_held_twice(units, (3,), (3, 3)))["rows"]
    weights, adjacency, want = gu.groups_table(n, rows)
    return n, weights, adjacency, rows, want


def test_groups_primitive_on_any_adjacency_on_a_stream_of_the_callers():
    n, weights, adjacency, rows, want = _groups_case()
    b = _groups_buffers(n, weights, adjacency, rows)
    stream = nat.Stream()
    rounds = _groups_call(b, stream)
    assert _groups_call(b, stream) == rounds >= 2
    stream.synchronize()
    got = _groups_result(b)
    for f in want:
        assert ints(got[f]) == want[f], f
    assert 1 < len(want["head"]) < n
    # no edge of either kind: every unit its own group, and no round
    empty = _groups_buffers(5, [7] * 5, [[]] * 5, [])
    assert _groups_call(empty) == 0
    nat.synchronize()
    got = _groups_result(empty)
    assert ints(got["group_of"]) == ints(got["head"]) == [0, 1, 2, 3, 4] and ints(got["units"]) == [1] * 5 and ints(got["weight"]) == [7] * 5


def test_groups_work_space_short_or_misaligned_is_refused_not_launched():
    n, weights, adjacency, rows, want = _groups_case()
    b = _groups_buffers(n, weights, adjacency, rows)
    nat.check(nat.lib().dcrx_memset_device(b["out"][4].ptr, 0xAB, 4))
    for kwargs in ({"short": 1}, {"shift": 8}):
        with pytest.raises(nat.DcrxError) as e:
            _groups_call(b, **kwargs)
        assert e.value.code == E_INVALID
    nat.synchronize()
    assert int(b["out"][4].to_host(np.uint32, 1)[0]) == 0xABABABAB      # nothing ran
    _groups_call(b, shift=256)
    nat.synchronize()
    assert ints(_groups_result(b)["group_of"]) == want["group_of"]


# ---- the host entry's refusals ----

def test_selected_motifs_out_of_order_or_outside_k_are_refused():
    units = list(_pool()[:20])
    off, text = spans(units)
    w = [1] * 20
    for ks, selected in (((2, 3), [(2, 5), (2, 5)]), ((2, 3), [(2, 5), (2, 4)]), ((2, 3), [(3, 0), (2, 0)]), ((2, 3), [(4, 0)]), ((2,), [(3, 7)]),
                         ((2, 3), [(2, 26 * 26)]), ((2, 3), [(5, 0)])):
        with pytest.raises(gu.Invalid):
            gu.expected_groups(units, w, ks, (3, 3), selected, 1)
        with pytest.raises(nat.DcrxError) as e:
            nat.cdr3_motif_groups(off, text, w, ks, (3, 3), [k for k, _ in selected], [c for _, c in selected], 1)
        assert e.value.code == E_INVALID, selected
    for kwargs in ({"trim": (17, 0)}, {"distance": 3}):
        with pytest.raises(nat.DcrxError) as e:
            nat.cdr3_motif_groups(off, text, w, **dict({"ks": (2,), "trim": (3, 3), "sel_k": [], "sel_code": [], "distance": 1}, **kwargs))
        assert e.value.code == E_INVALID
    down = np.array(off, np.uint64)
    down[3], down[4] = down[4], down[3]
    with pytest.raises(nat.DcrxError) as e:
        nat.cdr3_motif_groups(down, text, w, (2,), (3, 3), [], [], 1)
    assert e.value.code == E_INVALID and "offsets" in str(e.value)


def test_members_fit_the_callers_room_or_are_left_out():
    units, selected = _members_case()
    off, text = spans(units)
    args = (off, text, [1] * len(units), (2, 3), (3, 3), [k for k, _ in selected], [c for _, c in selected], 1)
    whole = nat.cdr3_motif_groups(*args)
    short = nat.cdr3_motif_groups(*args, mem_cap=whole["need"] - 1)
    assert short["need"] == whole["need"] and len(short["mem"]) == 0 and ints(short["group_of"]) == ints(whole["group_of"])
    gu.assert_same(nat.cdr3_motif_groups(*args, mem_cap=whole["need"]), whole)
    gu.assert_same(short, gu.expected_groups(units, [1] * len(units), (2, 3), (3, 3), selected, 1, mem_cap=whole["need"] - 1))


# ---- one random table, and the sub-command ----

def test_random_table_of_2000_with_the_motifs_of_a_real_run():
    pool = mu.random_units(6000, 77, 8, 14)
    base = list(pool[:1520])
    units = list(dict.fromkeys(mu.planted(base[:400], b"GTD", 4, 60) + base[400:] + _mutants(base[:500], 5)))[:2000]
    assert len(units) == 2000
    s_off, s_text = spans(units)
    b_off, b_text = spans(list(pool[1520:]))
    found = nat.cdr3_motifs(s_off, s_text, b_off, b_text, (2, 3, 4), (3, 3), 3, 50, 1)
    rows = motifs.selected_rows(found, 50, motifs.parse_decimal("0.02"), motifs.parse_decimal("2"))
    selected = [(int(found["k"][r]), int(found["code"][r])) for r in rows]
    assert (3, mu.code_of(b"GTD")) in selected and len(selected) > 20
    got, _ = _check(units, selected, G=1)
    assert got["stats"]["global_edges"] > 300 and got["stats"]["mixed_groups"] > 0 and got["need"] > 2 * len(selected)


def test_sub_command_end_to_end(tmp_path):
    g, bg = str(tmp_path / "G.clonotypes.tsv"), str(tmp_path / "naive.clonotypes.tsv")
    mu.clonotype_file(g, cpu.G_SAMPLE, repeat_first=2)
    mu.clonotype_file(bg, cpu.G_BACKGROUND)
    out = str(tmp_path) + "/"
    pipeline.main(["motifs", "-in", g, "-bg", bg, "-op", out, "-dz", "--motif-min-count", "2", "--motif-k", "2,3", "--resamples", "20",
                   "--groups", "--group-p-value", "0.05", "--write-motif-members"])
    units = motifs.units_of(cpu.G_SAMPLE)
    found = mu.expected_motifs(cpu.G_SAMPLE, cpu.G_BACKGROUND, (2, 3), (3, 3), 2, 20, 1)
    selected = [(int(found["k"][r]), int(found["code"][r])) for r in gu.selected_rows(found, 20, "0.05", "10")]
    rows_of, reads_of = [2, 2, 1, 1, 1, 1, 1, 1], [3, 3, 1, 1, 1, 1, 1, 1]
    want = gu.expected_groups(units, reads_of, (2, 3), (3, 3), selected, 1)
    lines = open(out + "dcr_G.cdr3_groups.tsv").read().split("\n")
    assert lines[0] == cpu.GROUPS_HEAD and lines[-1] == "" and lines[1:-1] == gu.groups_lines(units, rows_of, reads_of, want, selected)
    lines = open(out + "dcr_G.cdr3_motif_members.tsv").read().split("\n")
    assert lines[0] == cpu.MEMBERS_HEAD and lines[-1] == "" and lines[1:-1] == gu.member_lines(units, want, selected, (3, 3))
    assert len(selected) == 7 and motifs.stats["G"]["reported"] == 7
