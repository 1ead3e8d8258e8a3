"""Gene-family tag sets (oracle/family.py) on the CPU: the generator's own guarantees, and the host emulation of the
device's per-read code against the oracle on reads whose tag windows lie within Hamming 1 of two tags and on the
decoy ladder.  The conditions that keep the GPU tests of tests/test_gpu_family_tagsets.py from passing on nothing
are asserted here on the same generators, from the oracle's results and the generator's marks."""
import numpy as np
import pytest

from decombinator_amd import _native as nat
from oracle import family
from tests import family_util as fu
from tests import parity_util as pu

SPLITS = ["original", "extended"]
N_CONTESTED, N_LADDER = 6000, 2000


@pytest.mark.parametrize("split", SPLITS)
def test_generator_guarantees(split):
    ts = fu.tagset(split)
    rep = family.check_family_tagset(ts)           # distances, shared halves, shuffled families, regions
    for gene, tags, fams in (("v", ts.v_tags, ts.v_families), ("j", ts.j_tags, ts.j_families)):
        assert len({len(t) for t in tags}) == 1
        assert all(3 <= len(f) <= 6 for f in fams) and rep[gene]["d1"] >= 2 and rep[gene]["d2"] >= 4
        in_fam = {m for f in fams for m in f}
        for a in range(len(tags)):
            for b in range(a + 1, len(tags)):
                d = family.hamming(tags[a], tags[b])
                assert d >= 1 and (d >= 3 or (a in in_fam and b in in_fam))
    # a half-tag keyword of a family maps to three or more tags
    vs, js = ts.half_splits
    for tags, fams, s in ((ts.v_tags, ts.v_families, vs), (ts.j_tags, ts.j_families, js)):
        for f, fam in enumerate(fams):
            half = tags[fam[0]][:s] if f % 2 == 0 else tags[fam[0]][s:]
            assert sum((t[:s] if f % 2 == 0 else t[s:]) == half for t in tags) == len(fam) >= 3
    # two thirds of the V regions carry a half tag 12-50 nt upstream of their tag (some more by the families' ancestors)
    halves = {t[:vs] for t in ts.v_tags} | {t[vs:] for t in ts.v_tags}
    with_decoy = sum(any(h in reg[len(reg) - jump - 50:len(reg) - jump] for h in halves)
                     for reg, jump in zip(ts.v_regions, ts.v_jumps))
    assert with_decoy >= len(ts.v_tags) // 2
    info = pu.native_tables(fu.tagset_dict(ts)).info()
    assert info["equal_len_per_automaton"] and info["v2_tables"], info


def test_generator_is_deterministic_in_its_arguments():
    a, b = family.make_family_tagset(7, "extended", "a"), family.make_family_tagset(7, "extended", "a")
    assert fu.tagset_dict(a) == fu.tagset_dict(b) and a.v_families == b.v_families and a.j_families == b.j_families
    c = family.make_family_tagset(8, "extended", "a")
    assert c.v_tags != a.v_tags
    plain = family.make_family_tagset(7, "extended", "a", related_regions=False, decoys=False)
    assert plain.v_tags == a.v_tags and plain.v_regions != a.v_regions
    r1, m1 = family.contested_reads(a, np.random.default_rng(3), 200)
    r2, m2 = family.contested_reads(b, np.random.default_rng(3), 200)
    assert r1 == r2 and m1.tobytes() == m2.tobytes()
    assert family.decoy_ladder(a, np.random.default_rng(3), 100)[0] == family.decoy_ladder(b, np.random.default_rng(3), 100)[0]


def test_is_contested_counts_the_tags_around_a_settled_window():
    w = fu.contested("original", N_CONTESTED)
    orec, _ = w.want("forward")
    nv, nj = family.contested_counts(w.ts, w.sense, orec)
    for i in list(range(0, 300)):
        assert family.is_contested(w.ts, w.sense[i], orec[i]) == (int(nv[i]), int(nj[i]))
    ok = orec["status"] == 0
    assert (nv[ok] >= 1).all() and (nj[ok] >= 1).all() and not nv[~ok].any()


@pytest.mark.parametrize("split", SPLITS)
def test_contested_workload_meets_its_conditions(split):
    """What the GPU tests rely on, at a tenth of their size: the shares as they stand, the counts scaled."""
    rep = fu.contested(split, N_CONTESTED).report
    print(rep)
    family.assert_contest_conditions(rep, scale=N_CONTESTED / 60_000)


@pytest.mark.parametrize("split", SPLITS)
def test_ladder_workload_meets_its_conditions(split):
    rep = fu.ladder_report(fu.ladder(split, N_LADDER))
    print(rep)
    fu.assert_ladder_conditions(rep, per_k=2000 * N_LADDER // 40_000)


@pytest.mark.parametrize("flags", [0, nat.F_V2_NO_LEAN_RESCUE, nat.F_V1_KERNELS, nat.F_LIST_RESCUE],
                         ids=["v2", "general-form-only", "three-launch", "listrescue"])
@pytest.mark.parametrize("orientation", ["reverse", "forward", "both"])
@pytest.mark.parametrize("split", SPLITS)
def test_emul_contested_reads_and_ladder_match_the_oracle(split, orientation, flags):
    be = pu.Backend("emul", fu.tagset_dict(fu.tagset(split)))
    fu.contested(split, N_CONTESTED).check(be, orientation, flags=flags, what="contested")
    fu.ladder(split, N_LADDER).check(be, orientation, flags=flags, what="ladder")


@pytest.mark.parametrize("split", SPLITS)
def test_emul_contested_reads_with_ns_allowed(split):
    be = pu.Backend("emul", fu.tagset_dict(fu.tagset(split)))
    fu.contested(split, N_CONTESTED).check(be, "both", allow_ns=True, what="contested, Ns allowed")


def test_family_fixture_is_what_the_generator_writes():
    """tests/golden/dcr_family_original_b.json.gz holds the generator's family set (its tags are near neighbours: the
    fixture's cases contest them), with the cases of casegen.family_cases among its labels."""
    import os
    from tests import golden_util as gu
    fx = gu.load(os.path.join(gu.GOLDEN_DIR, "dcr_family_original_b.json.gz"))
    tags = fx["tagset"]
    assert len(family.pairs_at(tags["v_tags"], 1)) >= 2 and len(family.pairs_at(tags["v_tags"], 2)) >= 4
    assert len(family.pairs_at(tags["j_tags"], 1)) >= 2 and len(family.pairs_at(tags["j_tags"], 2)) >= 4
    labels = {c["label"] for c in fx["cases"]}
    for want in ("v_midpoint", "j_midpoint", "v_near1_to_other", "j_near1_to_other", "v_midpoint_first_walk_fails",
                 "v_half1_decoy_first", "v_half1_decoy_last", "j_half2_decoy_first", "v_half2_upstream_of_half1",
                 "v_ladder_4", "v_ladder_5", "v_ladder_8", "v_ladder_9", "j_ladder_9", "v_midpoint_N_allowed", "mix"):
        assert want in labels, want
    # the reference counted verr* twice on a read whose first candidate's walk failed
    twice = [c for c in fx["cases"] if c["label"] == "v_midpoint_first_walk_fails"
             and c["counts"].get("verr1", 0) + c["counts"].get("verr2", 0) >= 2]
    assert twice
    # ... and settled windows within Hamming 1 of several tags on one of them, mostly the lowest index (a candidate whose
    # walk fails hands on to the next)
    ts = family.tagset_from_dict(tags)
    assert ts.half_splits == (tags["v_half_split"], tags["j_half_split"])
    several = lowest = 0
    for c in fx["cases"]:
        if c["label"] == "v_midpoint" and c["orientation"] == "forward" and c["expect"]:
            window = c["read"][c["expect"][5]:c["expect"][5] + len(ts.v_tags[0])]
            near = [g for g, t in enumerate(ts.v_tags) if family.hamming(window, t) <= 1]
            assert c["expect"][0] in near and len(near) >= 2, (c, near)
            several += 1
            lowest += c["expect"][0] == min(near)
    assert several >= 20 and lowest >= several // 2, (several, lowest)
    info = pu.native_tables({k: tags[k] for k in ("v_tags", "v_jumps", "v_regions", "j_tags", "j_jumps", "j_regions",
                                                  "v_half_split", "j_half_split")}).info()
    assert info["equal_len_per_automaton"] and info["v2_tables"], info
