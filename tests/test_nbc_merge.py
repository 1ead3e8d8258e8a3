"""The error merge of the barcode-free count (`--merge-errors`) on the CPU: the kernels' per-entry and per-pair code built by
g++ (tests/host_merge) against Python, hand-made tables and the constructed lists of nbc_merge_util through the contract
written in Python (nm.expected_merge) and through the host build, what the junction's definition is for on oracle-decombined
noisy clonal reads, and the stage with the oracle standing in for the count (nu.OracleCountDevice) and the brute force for
nat.merge_dcrs (nm.BruteMerge)."""
import gzip
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import io as dio
from decombinator_amd import pipeline, synth
from tests import chains_util as chu
from tests import nbc_count_util as nu
from tests import nbc_merge_util as nm
from tests import parity_util as pu


@pytest.fixture()
def stand_ins(monkeypatch):
    oc = nu.OracleCountDevice(monkeypatch)
    return oc, nm.BruteMerge(monkeypatch)


def _short_region_tagset():
    """config 2 with a V region and a J region shorter than the anchor."""
    ts = synth.config_tagset(2)
    v_regions, j_regions = list(ts.v_regions), list(ts.j_regions)
    v_regions[1], j_regions[1] = v_regions[1][-20:], j_regions[1][:17]
    v_regions[2] = v_regions[2][:-3] + "n" + v_regions[2][-2:]          # a window that is not clean
    return synth.TagSet(species=ts.species, tags=ts.tags, chain=ts.chain, v_tags=ts.v_tags, v_jumps=ts.v_jumps, v_names=ts.v_names,
                        v_regions=v_regions, j_tags=ts.j_tags, j_jumps=ts.j_jumps, j_names=ts.j_names, j_regions=j_regions)


def _decode(words, length):
    return "".join("ACGT"[(int(words[p // 16]) >> (2 * (p % 16))) & 3] for p in range(length))


def test_host_encode_and_distance_match_python():
    L = nm.host_merge_lib()
    assert L.merge_host_words() == 8 and L.merge_host_win_words() == 10
    ts = _short_region_tagset()
    rows = nm.host_windows(L, ts)
    nv = len(ts.v_regions)
    rng = np.random.default_rng(3)
    cases = []
    for it in range(6000):
        v, j = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        vdel = int(rng.choice([0, 0, 3, 10, 20, 31, 32, 33, 40, 255]))
        jdel = int(rng.choice([0, 0, 2, 12, 17, 18, 32, 33, 200]))
        kind = rng.integers(0, 8)
        ln = int(rng.choice([0, 0, 1, 5, 12, 25, 64, 65, 66, 100, 128, 129]))
        ins = "".join(rng.choice(list("ACGT"), size=ln))
        if kind == 0 and ln:
            ins = ins[:ln // 2] + rng.choice(list("acgtNRYKMSW")) + ins[ln // 2 + 1:]
        cases.append((v, j, vdel, jdel, ins))
    # junctions of exactly 128 and 129 bases
    for extra in (64, 65):
        cases.append((0, 0, 0, 0, "ACGT" * 16 + "A" * (extra - 64)))
    seen = {"reach": 0, "out": 0, 128: 0, 129: 0}
    enc = []
    for v, j, vdel, jdel, ins in cases:
        want, ok = nm.junction_of(ts, v, j, vdel, jdel, ins)
        buf = np.frombuffer(ins.encode("latin-1") + b"\0", np.uint8)
        out, length = np.zeros(8, np.uint32), C_u32()
        got = L.merge_host_encode(rows[v].ctypes.data, rows[nv + j].ctypes.data, vdel, jdel, buf.ctypes.data, len(ins), out.ctypes.data,
                                  length.ctypes.data)
        assert bool(got) == ok, (v, j, vdel, jdel, ins)
        if ok:
            assert int(length[0]) == len(want) and _decode(out, len(want)) == want, (v, j, vdel, jdel, ins)
            assert all(int(out[w]) >> (2 * max(0, len(want) - 16 * w)) == 0 for w in range(8) if len(want) < 16 * (w + 1))
            enc.append((want, out.copy()))
            seen["reach"] += 1
            seen[len(want)] = seen.get(len(want), 0) + 1
        else:
            assert int(length[0]) == 0 and not out.any()
            seen["out"] += 1
            full = ts.v_regions[v].upper()[-32:][:max(0, min(32, len(ts.v_regions[v])) - vdel)] + ins + ts.j_regions[j].upper()[:32][jdel:]
            if len(full) == 129 and vdel <= 32 and jdel <= 32:
                seen[129] += 1
    assert seen["reach"] > 500 and seen["out"] > 500 and seen[128] >= 1 and seen[129] >= 1
    by_len = {}
    for s, w in enc:
        by_len.setdefault(len(s), []).append((s, w))
    pairs = 0
    for group in by_len.values():
        for a in range(0, len(group) - 1):
            (sa, wa), (sb, wb) = group[a], group[a + 1]
            ham = sum(x != y for x, y in zip(sa, sb))
            for limit in (1, 2):
                d = L.merge_host_distance(wa.ctypes.data, wb.ctypes.data, limit)
                assert (d == ham) if ham <= limit else (d > limit)
            pairs += 1
    # close pairs: one and two substitutions of one junction
    for s, w in enc[:300]:
        if len(s) < 2:
            continue
        for nsub in (1, 2, 3):
            t = list(s)
            for p in rng.choice(len(s), size=min(nsub, len(s)), replace=False):
                t[p] = "ACGT"[("ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) % 4]
            w2 = np.zeros(8, np.uint32)
            for p, c in enumerate(t):
                w2[p // 16] |= np.uint32("ACGT".index(c) << (2 * (p % 16)))
            ham = sum(x != y for x, y in zip(s, t))
            d = L.merge_host_distance(w.ctypes.data, w2.ctypes.data, 2)
            assert (d == ham) if ham <= 2 else (d > 2)
    assert pairs > 300


def C_u32():
    return np.zeros(1, np.uint32)


def _check_table(ts, counted, D, R):
    """expected_merge and the host build agree on the parents' consequences; returns expected_merge's result."""
    out, stats, root_of = nm.expected_merge(counted, ts, D, R)
    parent, reach = nm.host_parents(nm.host_merge_lib(), ts, counted, D, R)
    assert np.array_equal(nm.roots_of(parent), root_of)
    assert int((reach == 0).sum()) == stats["out_of_reach"]
    assert int(out["count"].sum()) == int(counted["count"].sum())
    return out, stats, root_of


def _sub(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def test_hand_made_tables():
    ts = synth.config_tagset(2)
    A = "ACGTTGCAAGGT"
    # a chain c -> p -> q: c is two substitutions from q
    t = nm.ranked([(0, 0, 3, 2, A, 1000, 5), (0, 0, 3, 2, _sub(A, 4), 50, 9), (0, 0, 3, 2, _sub(_sub(A, 4), 7), 2, 11)])
    out, stats, root = _check_table(ts, t, 1, 10)
    assert root.tolist() == [0, 0, 0] and stats["longest_chain"] == 2 and stats["merged"] == 2 and stats["reads_moved"] == 52
    assert nat.count_rows(out) == [["0", "0", "3", "2", A, 1052]] and int(out["first"][0]) == 5
    # two eligible parents (the child is one substitution from either): the lower rank wins
    B = _sub(A, 1)
    t = nm.ranked([(0, 0, 3, 2, A, 900, 0), (0, 0, 3, 2, _sub(_sub(A, 9), 10), 800, 1), (0, 0, 3, 2, _sub(A, 9), 3, 2)])
    out, stats, root = _check_table(ts, t, 1, 10)
    assert root.tolist() == [0, 1, 0]
    # the ratio's edge
    for cp, merges in ((30, True), (29, False)):
        t = nm.ranked([(1, 1, 0, 0, A, cp, 0), (1, 1, 0, 0, B, 3, 1)])
        assert _check_table(ts, t, 1, 10)[2].tolist() == ([0, 0] if merges else [0, 1])
    # R = 1 with equal counts: the rank decides
    t = nm.table([(1, 1, 0, 0, A, 7, 4), (1, 1, 0, 0, B, 7, 6)])
    out, stats, root = _check_table(ts, t, 1, 1)
    assert root.tolist() == [0, 0] and nat.count_rows(out) == [["1", "1", "0", "0", A, 14]]
    # the same substitution seen as a different (vdel, insert) pair: the read's last germline V base was substituted, the
    # deletion walk made it vdel + 1 and put the base in front of the insert
    Vr = ts.v_regions[2].upper()
    vend = Vr[len(Vr) - 3 - 1]                                   # the germline base the child gave up
    t = nm.ranked([(2, 0, 3, 0, A, 500, 0), (2, 0, 4, 0, "ACGT"[("ACGT".index(vend) + 1) % 4] + A, 4, 1)])
    assert _check_table(ts, t, 1, 10)[2].tolist() == [0, 0]
    # a different length does not merge
    t = nm.ranked([(2, 0, 3, 0, A, 500, 0), (2, 0, 3, 0, A + "A", 4, 1), (2, 1, 3, 0, _sub(A, 2), 4, 2)])
    assert _check_table(ts, t, 2, 1)[2].tolist() == [0, 1, 2]
    # out-of-reach entries pass through and are no one's parent
    t = nm.ranked([(0, 0, 3, 2, A[:5] + "N" + A[6:], 900, 0), (0, 0, 3, 2, A, 40, 1), (0, 0, 3, 2, A[:5] + "a" + A[6:], 2, 2),
                   (0, 0, 3, 2, _sub(A, 0), 2, 3), (0, 0, 40, 2, A, 1, 4)])
    out, stats, root = _check_table(ts, t, 1, 10)
    assert root.tolist() == [0, 1, 2, 1, 4] and stats["out_of_reach"] == 3 and stats["roots_out"] == 4
    # D = 2
    t = nm.ranked([(0, 0, 3, 2, A, 100, 0), (0, 0, 3, 2, _sub(_sub(A, 1), 8), 5, 1), (0, 0, 3, 2, _sub(_sub(_sub(A, 1), 8), 11), 5, 2)])
    assert _check_table(ts, t, 2, 10)[2].tolist() == [0, 0, 2]
    assert _check_table(ts, t, 1, 10)[2].tolist() == [0, 1, 2]
    # the order of the output: a merged count overtakes
    t = nm.ranked([(0, 0, 3, 2, A, 100, 3), (1, 0, 3, 2, A, 99, 1), (1, 0, 3, 2, _sub(A, 3), 9, 0)])
    out, stats, root = _check_table(ts, t, 1, 10)
    assert nat.count_rows(out) == [["1", "0", "3", "2", A, 108], ["0", "0", "3", "2", A, 100]] and out["first"].tolist() == [0, 3]
    # nothing at all
    out, stats, root = nm.expected_merge(nm.table([]), ts, 1, 10)
    assert len(out["v"]) == 0 and stats["roots_out"] == 0 and len(root) == 0


# ---- the constructed lists of nbc_merge_util (the builders assert each list's premise; here the host build agrees with the
# contract on them, before a GPU sees them in test_gpu_nbc_merge.py) ----

def _twin(ts, counted, D, R):
    """_check_table, and the host build's parents and reach flags against the contract's, entry by entry."""
    out, stats, root_of = _check_table(ts, counted, D, R)
    parent, reach = nm.host_parents(nm.host_merge_lib(), ts, counted, D, R)
    want_parent, want_reach = nm.expected_parents(counted, ts, D, R)
    assert parent.tolist() == want_parent and reach.astype(bool).tolist() == want_reach
    return out, stats, root_of


@pytest.mark.parametrize("n_fill", nm.DECOY_FILLERS)
def test_list_padding_decoys(n_fill):
    ts = synth.config_tagset(2)
    for length in nm.DECOY_LENGTHS:
        for with_children in (False, True):
            counted, merges = nm.padding_decoys(ts, length, n_fill, with_children)
            assert _twin(ts, counted, 2, 1)[1]["merged"] == merges


def test_list_gene_pair_decoys():
    ts = synth.config_tagset(2)
    for axis in "vj":
        for D, R in ((1, 10), (2, 1)):
            _twin(ts, nm.gene_pair_decoys(ts, axis), D, R)


@pytest.mark.parametrize("R", [1, 2, 10])
def test_list_prefix_ends(R):
    ts = synth.config_tagset(2)
    for k, gap in nm.PREFIX_PLACES:
        for eligible in (True, False):
            counted, child, want = nm.prefix_end(ts, R, k, gap, eligible)
            for D in (1, 2):
                assert nm.host_parents(nm.host_merge_lib(), ts, counted, D, R)[0][child] == want
                _twin(ts, counted, D, R)


def test_list_equal_counts_deep_chain_and_lengths():
    ts = synth.config_tagset(2)
    ball = nm.equal_counts_ball(ts)
    edges, _ = nm.lengths_and_word_edges(ts)
    for D in (1, 2):
        _twin(ts, ball, D, 1)
        for n_out in (0, 200):
            assert _twin(ts, nm.deep_chain(ts, n_out), D, 1)[1]["longest_chain"] == nm.CHAIN_LINKS // D
        for R in (10, 1):
            _twin(ts, edges, D, R)
    _twin(_short_region_tagset(), nm.short_window_mix(_short_region_tagset()), 1, 10)


def test_list_big_and_zero_counts():
    ts = synth.config_tagset(2)
    for name, counted, D, R, roots in nm.big_counts(ts):
        assert _twin(ts, counted, D, R)[2].tolist() == roots, name
    for D, R in ((1, 10), (2, 1), (1, nm.U64)):
        _twin(ts, nm.zero_counts(ts), D, R)
    nm.primitive_defects(ts)          # (its premises; the defects themselves are the device primitive's rules)


def test_substituted_reads_join_their_clone():
    """What the junction's definition is for.  Every read with exactly one substitution, inside the junction span, whose DCR
    is OK with its clone's v and j and in reach, shares its clone's root (D = 1) whenever the clone's pristine DCR is in
    reach and has count // R >= that DCR's count.  400 pristine clones, Zipf 1.2, 200 000 reads, 0.005 substitutions per
    base, R = 10: 13 029 reads meet the premise (asserted to be at least 500, and printed), over 9 045 distinct DCRs of which
    none is out of reach."""
    ts = synth.config_tagset(2)
    D, R = 1, 10
    reads, clone, places, pool = nm.noisy_clonal_reads(ts, 200_000, seed=77, n_pool=400, zipf=1.2, sub_rate=0.005, orientation="forward")
    ot = nu.oracle_for(ts)
    keys, _ = nu.read_dcrs(ot, reads, "forward")
    pool_keys, _ = nu.read_dcrs(ot, pool, "forward")
    pool_rec, _ = pu.oracle_records(ot, pool, "forward", False, 130)
    counted = nm.counted_from_keys(keys)
    assert nm.out_of_reach_share(counted, ts) <= 0.01
    out, stats, root_of = nm.expected_merge(counted, ts, D, R)
    assert int(out["count"].sum()) == sum(1 for k in keys if k)
    rows = [", ".join(r[:5]) for r in nat.count_rows(counted)]
    rank = {k: i for i, k in enumerate(rows)}
    count = counted["count"].tolist()

    def reach(key):
        f = key.split(", ")
        return nm.junction_of(ts, int(f[0]), int(f[1]), int(f[2]), int(f[3]), f[4])[1]

    met = 0
    for k, key in enumerate(keys):
        if key is None or len(places[k]) != 1:
            continue
        c = int(clone[k])
        pk, pr = pool_keys[c], pool_rec[c]
        if pk is None or pk not in rank or int(pr["frame"]) != 1:
            continue
        f, pf = key.split(", "), pk.split(", ")
        if f[:2] != pf[:2] or not reach(key) or not reach(pk):
            continue
        aV = min(32, len(ts.v_regions[int(pf[0])]))
        aJ = min(32, len(ts.j_regions[int(pf[1])]))
        lo = int(pr["ins_start"]) - (aV - int(pr["vdel"]))
        hi = int(pr["ins_start"]) + int(pr["ins_len"]) + (aJ - int(pr["jdel"]))
        if not lo <= int(places[k][0]) < hi:
            continue
        if count[rank[pk]] // R < count[rank[key]]:
            continue
        met += 1
        assert root_of[rank[key]] == root_of[rank[pk]], (key, pk)
    print(f"{met} reads met the premise; {len(rows)} DCRs, {stats}")
    assert met >= 500


def _argv(tmp_path, ts, reads, extra=()):
    return nu.workdir_with(tmp_path, ts, reads) + ["--merge-errors"] + list(extra)


def _noisy(ts, n=6000, seed=5, **kw):
    return nm.noisy_clonal_reads(ts, n, seed=seed, n_pool=40, sub_rate=0.004, **kw)[0]


def _want(ts, reads, D=1, R=10, orientation="reverse"):
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads, orientation)
    counted = nm.counted_from_keys(keys)
    out, stats, root_of = nm.expected_merge(counted, ts, D, R)
    return counted, out, stats, root_of, sum(1 for k in keys if k)


def _merges_text(counted, root_of):
    rows = nat.count_rows(counted)
    return "".join(", ".join(rows[k][:5] + [str(rows[k][5])] + rows[int(root_of[k])][:5]) + "\n"
                   for k in range(len(rows)) if root_of[k] != k)


def test_refusals_before_anything_is_read(tmp_path, monkeypatch, stand_ins, capsys):
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    base = ["-in", "TINY_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "-nbc"]
    for argv, msg in ((["decombine"] + base + ["--merge-errors"], "needs --count-dcrs"),
                      (["pipeline"] + base + ["--merge-errors"], "needs --count-dcrs"),
                      (["decombine"] + base + ["--count-dcrs", "--merge-distance", "1"], "only with --merge-errors"),
                      (["decombine"] + base + ["--count-dcrs", "--merge-ratio", "10"], "only with --merge-errors"),
                      (["pipeline"] + base + ["--count-dcrs", "--write-merges"], "only with --merge-errors"),
                      (["decombine"] + base + ["--count-dcrs", "--merge-errors", "--merge-distance", "3"], "1 or 2"),
                      (["decombine"] + base + ["--count-dcrs", "--merge-errors", "--merge-distance", "0"], "1 or 2"),
                      (["pipeline"] + base + ["--count-dcrs", "--merge-errors", "--merge-ratio", "0"], ">= 1"),
                      (["decombine"] + base[:-1] + ["--count-dcrs", "--merge-errors"], "needs -nbc")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
        assert msg in capsys.readouterr().err, argv
    for cmd in ("collapse", "translate"):
        with pytest.raises(SystemExit):
            pipeline.main([cmd, "-in", "x.n12", "-c", "b", "--merge-errors"])
    capsys.readouterr()
    d = dio.create_args_dict(infile="x", chain="b", bc_read="R2")
    assert (d["merge_errors"], d["merge_distance"], d["merge_ratio"], d["write_merges"]) == (False, 1, 10, False)
    args = dio.create_args_dict(infile="TINY_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", nobarcoding=True)
    for kw, msg in ((dict(merge_errors=True), "needs --count-dcrs"), (dict(count_dcrs=True, merge_distance=2), "only with"),
                    (dict(count_dcrs=True, merge_ratio=3), "only with"), (dict(count_dcrs=True, write_merges=True), "only with"),
                    (dict(count_dcrs=True, merge_errors=True, merge_distance=3), "1 or 2"),
                    (dict(count_dcrs=True, merge_errors=True, merge_ratio=0), ">= 1"),
                    (dict(count_dcrs=True, merge_errors=True, merge_ratio=2.5), ">= 1")):
        with pytest.raises(ValueError, match=msg):
            dec.decombinator(dict(args, **kw))
        with pytest.raises(ValueError, match=msg):
            dec.decombinator_chains(dict(args, chain="a,b", **kw))
    assert stand_ins[1].calls == []


def test_stage_files_plain_and_gzipped(tmp_path, monkeypatch, stand_ins):
    monkeypatch.chdir(tmp_path)
    ts = synth.config_tagset(2)
    reads = _noisy(ts)
    counted, out, stats, root_of, n_ok = _want(ts, reads)
    assert stats["merged"] > 20 and stats["roots_out"] >= 20
    want_nbc, want_merges = nu.counted_text(out), _merges_text(counted, root_of)
    assert want_merges.count("\n") == stats["merged"]
    for d, extra, names in (("plain", ["-dz", "--write-merges"], ["dcr_NBC_1_beta.merges", "dcr_NBC_1_beta.nbc"]),
                            ("gz", ["--write-merges"], ["dcr_NBC_1_beta.merges.gz", "dcr_NBC_1_beta.nbc.gz"]),
                            ("only", ["-dz"], ["dcr_NBC_1_beta.nbc"]),
                            ("ext", ["-dz", "-ex", "dcrs", "-pf", "x_", "--write-merges"], ["x_NBC_1_beta.dcrs", "x_NBC_1_beta.merges"])):
        (tmp_path / d).mkdir()
        pipeline.main(["decombine"] + _argv(tmp_path, ts, reads, extra) + ["-op", f"{d}/"])
        assert sorted(x for x in os.listdir(tmp_path / d) if x != "Logs") == names
        for name in names:
            p = tmp_path / d / name
            got = (gzip.open(p).read() if name.endswith(".gz") else p.read_bytes()).decode()
            assert got == (want_merges if ".merges" in name else want_nbc), name
            assert oct(os.stat(p).st_mode)[-3:] == "666"
        assert dec.merge_stats == stats
        assert sum(int(ln.split(", ")[5]) for ln in want_nbc.splitlines()) == dec.counts["vj_count"] == n_ok
    assert all(len(ln.split(", ")) == 6 for ln in want_nbc.splitlines())
    assert stand_ins[1].calls[0] == (len(counted["v"]), 1, 10)
    # other parameters reach the one call
    (tmp_path / "p").mkdir()
    pipeline.main(["decombine"] + _argv(tmp_path, ts, reads, ["-dz", "--merge-distance", "2", "--merge-ratio", "3"]) + ["-op", "p/"])
    assert stand_ins[1].calls[-1] == (len(counted["v"]), 2, 3)
    assert (tmp_path / "p" / "dcr_NBC_1_beta.nbc").read_text() == nu.counted_text(nm.expected_merge(counted, ts, 2, 3)[0])


def test_summary_lines_only_with_the_flag(tmp_path, monkeypatch, stand_ins):
    monkeypatch.chdir(tmp_path)
    ts = synth.config_tagset(2)
    reads = _noisy(ts, 3000, seed=8)
    counted, out, stats, root_of, n_ok = _want(ts, reads)
    pipeline.main(["decombine"] + nu.workdir_with(tmp_path, ts, reads) + ["-dz", "-op", "a/"])
    plain = chu.log_lines(next((tmp_path / "a" / "Logs").glob("*Summary.csv")))
    assert dec.merge_stats == {} and not any("Merge" in ln for ln in plain)
    assert (tmp_path / "a" / "dcr_NBC_1_beta.nbc").read_text() == nu.counted_text(counted)
    pipeline.main(["decombine"] + _argv(tmp_path, ts, reads, ["-dz", "-op", "b/"]))
    merged = chu.log_lines(next((tmp_path / "b" / "Logs").glob("*Summary.csv")))
    assert merged[:len(plain) - 1] == plain[:-1]          # (the last element is what follows the final newline)
    tail = [ln for ln in merged[len(plain) - 1:] if ln]
    assert tail == ["ErrorMerge:,", "MergeDistance,1", "MergeRatio,10", f"DCRsBeforeMerge,{stats['entries_in']}",
                    f"DCRsAfterMerge,{stats['roots_out']}", f"DCRsOutOfReach,{stats['out_of_reach']}",
                    f"DCRsMerged,{stats['merged']}", f"ReadsMoved,{stats['reads_moved']}",
                    f"LongestMergeChain,{stats['longest_chain']}"]


def test_both_chains_equal_single_runs(tmp_path, monkeypatch, stand_ins):
    monkeypatch.chdir(tmp_path)
    ta, tb = synth.config3_tagsets()
    reads = _noisy(ta, 3000, seed=12) + _noisy(tb, 3000, seed=13)
    np.random.default_rng(2).shuffle(reads)
    ta.write(str(tmp_path / "tags"))
    tb.write(str(tmp_path / "tags"))
    nu.write_fastq(tmp_path / "NBC_1.fq", reads)
    base = ["-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--merge-errors", "--write-merges", "-tfdir", "tags", "-tg", ta.tags,
            "-sp", ta.species, "-dc", "-dz"]
    got = chu.compare_with_single_runs(tmp_path, f"{ta.chain},{tb.chain}", base)
    files = sorted(k for k in got if not k.startswith("Logs"))
    assert len(files) == 4 and sum(f.endswith(".merges") for f in files) == 2
    for ts in (ta, tb):
        counted, out, stats, root_of, n_ok = _want(ts, reads)
        assert dec.chain_merge_stats[ts.chain] == stats and stats["merged"] > 5
        name = [f for f in files if f.endswith(".nbc") and dec.chainnams[ts.chain] in f][0]
        assert got[name].decode() == nu.counted_text(out)
    assert [c[0] for c in stand_ins[1].calls[:2]] == [len(_want(ts, reads)[0]["v"]) for ts in (ta, tb)]


def test_pipeline_counts_are_the_merged_counts(tmp_path, monkeypatch, stand_ins):
    monkeypatch.chdir(tmp_path)
    from tests.test_nbc_count import _translate_stubs, _tsv_rows
    _translate_stubs(monkeypatch)
    ts = synth.config_tagset(2)
    reads = _noisy(ts, 4000, seed=21, orientation="both")
    pipeline.main(["pipeline"] + _argv(tmp_path, ts, reads, ["-dz", "-or", "both", "--write-merges"]))
    counted, out, stats, root_of, n_ok = _want(ts, reads, orientation="both")
    assert (tmp_path / "dcr_NBC_1_beta.nbc").read_text() == nu.counted_text(out)
    assert (tmp_path / "dcr_NBC_1_beta.merges").read_text() == _merges_text(counted, root_of)
    rows = _tsv_rows(tmp_path / "dcr_NBC_1_beta.tsv")
    assert [int(r["duplicate_count"]) for r in rows] == out["count"].tolist()
    assert [r["sequence"] for r in rows] == ["|".join(r[:5]) for r in nat.count_rows(out)]
    assert sum(out["count"].tolist()) == dec.counts["vj_count"] == n_ok and stats["merged"] > 10


def test_c_abi_argument_errors():
    ts = synth.config_tagset(2)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    assert nat.ABI_VERSION == 5 and nat.lib().dcrx_abi_version() == 5
    assert nat.MERGE_ANCHOR == nm.ANCHOR and nat.MERGE_MAX_JUNCTION == nm.MAX_JUNCTION
    tab = nm.table([(0, 0, 1, 1, "ACGT", 5, 0)])
    for d, r, msg in ((0, 10, "1 or 2"), (3, 10, "1 or 2"), (1, 0, ">= 1")):
        with pytest.raises(nat.DcrxError, match=msg):
            nat.merge_dcrs(t, tab, d, r)
    # an empty table needs no device
    out, stats, root_of = nat.merge_dcrs(t, nm.table([]), 1, 10)
    assert len(out["v"]) == 0 and stats == dict.fromkeys(nat.MERGE_STATS, 0) and len(root_of) == 0
    assert nat.lib().dcrx_merge_work_bytes(1 << 31) == 0
    # the table of the roots, gathered on the host
    tab = nm.table([(0, 0, 1, 1, "ACGT", 5, 0), (1, 2, 3, 4, "", 4, 1), (2, 1, 0, 0, "GGa", 3, 2)])
    got = nat.merged_counts(tab, [2, 0], [9, 5], [1, 0])
    assert nat.count_rows(got) == [["2", "1", "0", "0", "GGa", 9], ["0", "0", "1", "1", "ACGT", 5]] and got["first"].tolist() == [1, 0]
