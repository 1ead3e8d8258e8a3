"""Stage 2 of `collapse` (--cluster) on the CPU: grouping, the protoseq test, the components and the counting are libdcrx's
host code and Python; the UMI neighbour search (a HIP kernel) is replaced by an independent brute force here
(tests/collapse_cluster_util.py), the pattern of test_host_stage.py's _oracle_device.  Expected outputs come from the
reference's own collapsinator (tests/golden/collapse_cluster.json) and its TINY `.freq` files (tests/golden/tiny_freq.json).
The search itself is checked here as far as a host can: dcrx_umi_encode's layout, and the kernel's tile rule, walk order and
pair function (dcrx_umi_core.h built by g++, tests/host_umi) against the brute force on constructed UMI lists."""
import json
import os
import random
import subprocess
import ctypes as C

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import collapse, pipeline, synth
from decombinator_amd import io as dio
from tests import collapse_cluster_util as cu

CASES = cu.cases()
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture()
def cpu_neighbours(monkeypatch):
    monkeypatch.setattr(nat, "umi_neighbours", cu.brute_neighbours)


@pytest.mark.parametrize("case", CASES, ids=[c["params"]["name"] for c in CASES])
def test_fixture_case_collapsinator(case, tmp_path, monkeypatch, cpu_neighbours):
    monkeypatch.chdir(tmp_path)
    cu.check_case(case, cu.run_case(case, tmp_path))


@pytest.mark.parametrize("case", CASES, ids=[c["params"]["name"] for c in CASES])
def test_fixture_case_cli(case, tmp_path, monkeypatch, cpu_neighbours):
    monkeypatch.chdir(tmp_path)
    cu.check_case(case, cu.run_case(case, tmp_path, via_cli=True))


def _tiny_rows_text(chain_name):
    fx = json.load(open(os.path.join(HERE, "golden", f"tiny_{chain_name}.json")))
    return fx, "".join(", ".join(r) + "\n" for r in fx["rows_with_reconstructed_tagset"])


@pytest.mark.parametrize("chain_name", ["alpha", "beta"])
def test_tiny_collapse_cluster_equals_reference_freq(chain_name, tmp_path, monkeypatch, cpu_neighbours):
    """The TINY `.n12` rows -> collapse --cluster -> the reference's dcr_TINY_1_<chain>.freq, line for line."""
    monkeypatch.chdir(tmp_path)
    fx, text = _tiny_rows_text(chain_name)
    (tmp_path / f"dcr_TINY_1_{chain_name}.n12").write_text(text)
    pipeline.main(["collapse", "-in", f"dcr_TINY_1_{chain_name}.n12", "-ol", "M13", "--cluster", "-dz", "-c", chain_name[0]])
    want = json.load(open(os.path.join(HERE, "golden", "tiny_freq.json")))[chain_name]
    assert (tmp_path / f"dcr_TINY_1_{chain_name}.freq").read_text().splitlines() == want
    assert any("Collapsing_Summary" in x for x in os.listdir(tmp_path / "Logs"))


def _oracle_decombine(fx):
    from tests import golden_util as gu
    from tests import parity_util as pu
    ot = gu.oracle_tables(fx["tagset"])

    def fake(tables, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0):
        return pu.oracle_records(ot, nat.unpack_reads(batch), orientation, allow_ns, lenthreshold)
    return fake


def tiny_pipeline(chain_name, tmp_path, monkeypatch):
    """pipeline --cluster over the TINY FASTQ pair (the reconstructed tag set of tiny_<chain>.json): the .n12, .freq and the
    .tsv.  The reconstructed tag set carries no translate gene tables, so cdr3translator is a stand-in that records the rows
    it was handed (the CDR3 step itself is test_translate_cdr3.py's)."""
    from decombinator_amd import translate
    handed = []
    monkeypatch.setattr(translate, "cdr3translator", lambda inputargs, data=None: handed.extend(list(data)) or [])
    fx = json.load(open(os.path.join(HERE, "golden", f"tiny_{chain_name}.json")))
    ts = fx["tagset"]
    t = synth.TagSet(species=ts["species"], tags=ts["tags"], chain=ts["chain"], v_tags=ts["v_tags"], v_jumps=ts["v_jumps"],
                     v_names=ts["v_names"], v_regions=ts["v_regions"], j_tags=ts["j_tags"], j_jumps=ts["j_jumps"],
                     j_names=ts["j_names"], j_regions=ts["j_regions"])
    t.write(str(tmp_path / "tags"))
    (tmp_path / "TINY_1.fq").write_text(fx["fastq_r1"])
    (tmp_path / "TINY_2.fq").write_text(fx["fastq_r2"])
    pipeline.main(["pipeline", "-in", "TINY_1.fq", "-c", ts["chain"], "-br", "R2", "-dz", "-dc", "-tfdir", str(tmp_path / "tags"),
                   "-ol", "M13", "--cluster"])
    return json.load(open(os.path.join(HERE, "golden", "tiny_freq.json")))[chain_name], handed


@pytest.mark.parametrize("chain_name", ["alpha", "beta"])
def test_tiny_pipeline_cluster_cpu(chain_name, tmp_path, monkeypatch, cpu_neighbours):
    monkeypatch.chdir(tmp_path)
    fx = json.load(open(os.path.join(HERE, "golden", f"tiny_{chain_name}.json")))
    monkeypatch.setattr(nat, "decombine", _oracle_decombine(fx))
    want, handed = tiny_pipeline(chain_name, tmp_path, monkeypatch)
    assert (tmp_path / f"dcr_TINY_1_{chain_name}.freq").read_text().splitlines() == want
    assert [", ".join(map(str, r)) for r in handed] == want
    assert (tmp_path / f"dcr_TINY_1_{chain_name}.n12").exists()
    assert (tmp_path / f"dcr_TINY_1_{chain_name}.tsv").exists()


def test_collapse_without_cluster_still_writes_n12u(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _, text = _tiny_rows_text("beta")
    (tmp_path / "dcr_TINY_1_beta.n12").write_text(text)
    pipeline.main(["collapse", "-in", "dcr_TINY_1_beta.n12", "-ol", "M13", "-dz", "-c", "b"])
    assert (tmp_path / "dcr_TINY_1_beta.n12u").exists()
    assert not (tmp_path / "dcr_TINY_1_beta.freq").exists()


def test_cluster_flag_defaults():
    assert dio.create_args_dict(infile="x", chain="b", bc_read="R2")["cluster"] is False
    assert dio.cli_args(["collapse", "-in", "x.n12", "--cluster"])["cluster"] is True
    assert dio.cli_args(["pipeline", "-in", "x.fq", "-br", "R2"])["cluster"] is False


def test_components_match_networkx_order():
    nx = pytest.importorskip("networkx")
    rng = random.Random(5)
    for trial in range(200):
        n = rng.choice([10, 60, 300, 2000])
        edges = sorted({tuple(sorted(rng.sample(range(n), 2))) for _ in range(rng.randrange(1, 3 * n))})
        G = nx.Graph()
        for i, j in edges:
            G.add_edge(i, j)
        want = [list(c) for c in nx.connected_components(G)]
        got, _ = collapse._components([e[0] for e in edges], [e[1] for e in edges])
        assert got == want


def test_host_equivalence_matches_dp():
    rng = random.Random(7)
    for _ in range(20000):
        a = "".join(rng.choice("ACGTN") for _ in range(rng.randrange(0, 60)))
        b = list(a)
        for _ in range(rng.randrange(0, 8)):
            op = rng.randrange(3)
            if op == 0 and b:
                b[rng.randrange(len(b))] = rng.choice("ACGT")
            elif op == 1:
                b.insert(rng.randrange(len(b) + 1), rng.choice("ACGT"))
            elif b:
                del b[rng.randrange(len(b))]
        b = "".join(b)
        frac = rng.choice([0.0, 0.05, 0.1, 0.2, 0.33, 1.0])
        want = cu.lev(a, b) <= len(min(a, b, key=len)) * frac
        assert nat.seqs_equivalent(a, b, frac) == want, (a, b, frac)


def _host_umi_lib():
    d = os.path.join(HERE, "host_umi")
    subprocess.check_call(["make", "-s", "-C", d])
    L = C.CDLL(os.path.join(d, "build", "libumi_host.so"))
    L.umi_host_pair_distance.restype = C.c_int32
    L.umi_host_pair_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.umi_host_tiles_may_match.restype = C.c_int
    L.umi_host_tiles_may_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.umi_host_walk.restype = C.c_uint64
    L.umi_host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64]
    return L


def test_kernel_pair_function_on_host_matches_dp():
    """The kernel's per-pair decision (dcrx_umi_core.h built by g++) against the DP on 10^5 pairs: lengths 1-24, N bytes,
    k 0-4."""
    L = _host_umi_lib()
    rng = random.Random(11)
    umis = []
    for _ in range(2000):
        base = "".join(rng.choice("ACGTN") for _ in range(rng.randrange(1, 25)))
        umis.append(base)
        for _ in range(rng.randrange(0, 4)):
            s = list(base)
            for _ in range(rng.randrange(1, 4)):
                op = rng.randrange(3)
                if op == 0:
                    s[rng.randrange(len(s))] = rng.choice("ACGTN")
                elif op == 1 and len(s) < 24:
                    s.insert(rng.randrange(len(s) + 1), rng.choice("ACGTN"))
                elif len(s) > 1:
                    del s[rng.randrange(len(s))]
            umis.append("".join(s))
    recs, _ = nat.umi_encode(umis)
    where = {int(r[14]): r for r in recs[:len(umis)]}           # record of each UMI (the records are sorted)
    n_checked = 0
    for _ in range(100000):
        i, j = rng.randrange(len(umis)), rng.randrange(len(umis))
        if rng.random() < 0.5:
            j = min(len(umis) - 1, i + rng.randrange(1, 4))   # often a family member
        k = rng.randrange(0, 5)
        a, b = np.ascontiguousarray(where[i]), np.ascontiguousarray(where[j])
        d = L.umi_host_pair_distance(a.ctypes.data, b.ctypes.data, k)
        want = cu.lev(umis[i], umis[j])
        assert (d <= k) == (want <= k), (umis[i], umis[j], k, d, want)
        if want <= k:
            assert d == want
        n_checked += 1
    assert n_checked == 100000


def test_kernel_pair_function_at_the_length_limits():
    """The same check where the lengths end: an empty UMI on either side, 24 symbols on both, and eight distinct byte values
    with \\x00 and \\xff among them (bit 23 of Myers' word, symbol code 7)."""
    L = _host_umi_lib()
    rng = random.Random(13)
    syms = "\x00ACGTN\xffS"
    full = ["".join(rng.choice(syms) for _ in range(24)) for _ in range(150)]
    umis = [""]
    for base in full:
        umis.append(base)
        for _ in range(3):                                            # still 24 long: substitutions only
            s = list(base)
            for _ in range(rng.randrange(1, 5)):
                s[rng.randrange(24)] = rng.choice(syms)
            umis.append("".join(s))
        s = list(base)                                                # and a shifted one: a deletion and an insertion
        del s[rng.randrange(24)]
        s.insert(rng.randrange(24), rng.choice(syms))
        umis.append("".join(s))
    umis += ["".join(rng.choice(syms) for _ in range(n)) for n in (1, 1, 2, 2, 3, 4, 23, 23) for _ in range(4)]
    assert len(set("".join(umis))) == 8
    recs, _ = nat.umi_encode(umis)
    where = {}
    for r in recs[:len(umis)]:
        where[int(r[14])] = np.ascontiguousarray(r)
    empty = umis.index("")
    pairs = [(empty, j) for j in range(len(umis))] + [(j, empty) for j in range(len(umis))]
    n24 = [i for i, u in enumerate(umis) if len(u) == 24]
    pairs += [(rng.choice(n24), rng.choice(n24)) for _ in range(4000)]
    pairs += [(i, min(len(umis) - 1, i + d)) for i in n24 for d in range(5)]               # family members
    seen = {"empty": 0, "full": 0, "full_near": 0}
    for i, j in pairs:
        want = cu.lev(umis[i], umis[j])
        for k in (0, 1, 2, 3, 4, 23, 24, 25):
            d = L.umi_host_pair_distance(where[i].ctypes.data, where[j].ctypes.data, k)
            assert (d <= k) == (want <= k), (umis[i], umis[j], k, d, want)
            if want <= k:
                assert d == want
        seen["empty"] += not (umis[i] and umis[j])
        seen["full"] += len(umis[i]) == 24 == len(umis[j])
        seen["full_near"] += len(umis[i]) == 24 == len(umis[j]) and 0 < want <= 4
    assert seen["empty"] > 1000 and seen["full"] > 4000 and seen["full_near"] > 300


# ---- the search around the pair function: dcrx_umi_encode's layout, the whole-tile skip rule and the upper-triangle walk,
# on the constructed lists of collapse_cluster_util (the lists the GPU tests give the kernel) ----

UMI_CASES = cu.umi_constructed_cases()
UMI_IDS = [c[0] for c in UMI_CASES]


def _check_encode_layout(umis):
    n = len(umis)
    recs, tiles = nat.umi_encode(list(umis))
    n_tiles = (n + 255) // 256
    assert recs.shape == (n_tiles * 256, 16) and tiles.shape == (n_tiles, 8)
    assert sorted(recs[:n, 14].tolist()) == list(range(n))                                 # every index once
    comp = recs[:, 12:14].copy().view(np.uint8).reshape(-1, 8).astype(np.int64)          # byte s = count of symbol s
    lens = recs[:, 11].astype(np.int64)
    for s in range(n):                                                                      # each record is its UMI
        u = umis[int(recs[s, 14])]
        assert lens[s] == len(u) and comp[s].sum() == len(u)
        assert sorted(c for c in comp[s].tolist() if c) == sorted(u.count(c) for c in set(u))
    order = [(int(lens[s]),) + tuple(comp[s].tolist()) for s in range(n)]
    assert order == sorted(order)                                                           # (length, composition)
    assert not recs[n:].any()                                                               # padding of the last tile
    for t in range(n_tiles):
        lo, hi = t * 256, min(n, t * 256 + 256)
        assert tiles[t, 6] == hi - lo and tiles[t, 7] == 0
        assert tiles[t, 0] == lens[lo:hi].min() and tiles[t, 1] == lens[lo:hi].max()
        assert tiles[t, 2:4].copy().view(np.uint8).tolist() == comp[lo:hi].min(axis=0).tolist()
        assert tiles[t, 4:6].copy().view(np.uint8).tolist() == comp[lo:hi].max(axis=0).tolist()


@pytest.mark.parametrize("name,umis,ks", UMI_CASES, ids=UMI_IDS)
def test_umi_encode_layout_on_constructed_lists(name, umis, ks):
    _check_encode_layout(umis)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513])
def test_umi_encode_layout_on_random_lists(n):
    rng = random.Random(n)
    _check_encode_layout(["".join(rng.choice(cu.UMI_SYMBOLS) for _ in range(rng.randrange(0, 25))) for _ in range(n)])


def _tile_of_index(recs, n):
    tile_of = np.zeros(n, dtype=np.int64)
    tile_of[recs[:n, 14]] = np.arange(n) // 256
    return tile_of


def _rejected(L, tiles, k):
    t = np.ascontiguousarray(tiles)
    return {(a, b) for a in range(len(t)) for b in range(a, len(t))
            if not L.umi_host_tiles_may_match(t[a].ctypes.data, t[b].ctypes.data, k)}


@pytest.mark.parametrize("name,umis,ks", UMI_CASES, ids=UMI_IDS)
def test_tile_skip_rule_is_sound(name, umis, ks):
    """No tile pair the rule rejects holds a pair of the brute force (one UMI in each tile), at k = 0, 1, 2, 3, 24."""
    L = _host_umi_lib()
    recs, tiles = nat.umi_encode(list(umis))
    tile_of = _tile_of_index(recs, len(umis))
    for k in (0, 1, 2, 3, 24):
        rejected = _rejected(L, tiles, k)
        if name in ("all_pairs", "families") and k <= 2:
            assert rejected                        # lengths 0 to 24 in one list: the first and the last tile are out of reach
        if not rejected:
            continue                               # (nothing to be wrong about; at k = 24 that is every list)
        keys = cu.brute_keys(umis, k)
        ti, tj = tile_of[(keys >> np.uint64(32)).astype(np.int64)], tile_of[(keys & np.uint64(0xFFFFFFFF)).astype(np.int64)]
        crossed = set(zip(np.minimum(ti, tj).tolist(), np.maximum(ti, tj).tolist()))
        assert not (crossed & rejected), (k, sorted(crossed & rejected))


def _reach_len_layout(umis, k):
    """What the by-length list is for, from the encode output and the brute force: tiles 0 and 1 each of one length, exactly k
    apart, and at least 256 expected pairs with one UMI in each."""
    recs, tiles = nat.umi_encode(list(umis))
    assert tiles[0, 0] == tiles[0, 1] == 10 and tiles[1, 0] == tiles[1, 1] == 10 + k and tiles[0, 6] == tiles[1, 6] == 256
    _crossing(umis, k, recs, 256)
    return tiles


def _reach_comp_layout(umis, k):
    """The by-composition list: the first element fixes the symbol codes (A, C, G, T = 0..3, N = 4), both tiles hold 12-mers
    only, their composition summaries are 2k apart in L1 (k in A, k in N), and at least 256 expected pairs cross them."""
    assert umis[0] == "AAACCCGGGTTT"
    recs, tiles = nat.umi_encode(list(umis))
    assert len(tiles) == 2 and (tiles[:, 0:2] == 12).all() and (tiles[:, 6] == 256).all()
    mn, mx = tiles[:, 2:4].copy().view(np.uint8).reshape(2, 8).astype(int), tiles[:, 4:6].copy().view(np.uint8).reshape(2, 8).astype(int)
    assert (mn == mx).all()                                                                 # one composition per tile
    assert mn[0].tolist() == [3 - k, 3, 3, 3, k, 0, 0, 0] and mn[1].tolist() == [3, 3, 3, 3, 0, 0, 0, 0]
    assert np.abs(mn[0] - mn[1]).sum() == 2 * k
    _crossing(umis, k, recs, 256)
    return tiles


def _crossing(umis, k, recs, at_least):
    tile_of = _tile_of_index(recs, len(umis))
    keys = cu.brute_keys(umis, k)
    ti, tj = tile_of[(keys >> np.uint64(32)).astype(np.int64)], tile_of[(keys & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    assert int(((np.minimum(ti, tj) == 0) & (np.maximum(ti, tj) == 1)).sum()) >= at_least


@pytest.mark.parametrize("k", [1, 2])
def test_tile_skip_rule_accepts_tiles_exactly_at_reach(k):
    """Length gap = k, composition gap = 2k: in reach, and out of reach at k - 1."""
    L = _host_umi_lib()
    for tiles in (_reach_len_layout(cu.umi_reach_len_list(k), k), _reach_comp_layout(cu.umi_reach_comp_list(k), k)):
        t = np.ascontiguousarray(tiles)
        assert L.umi_host_tiles_may_match(t[0].ctypes.data, t[1].ctypes.data, k)
        assert L.umi_host_tiles_may_match(t[1].ctypes.data, t[0].ctypes.data, k)
        assert not L.umi_host_tiles_may_match(t[0].ctypes.data, t[1].ctypes.data, k - 1)


@pytest.mark.parametrize("name,umis,ks", UMI_CASES, ids=UMI_IDS)
def test_host_walk_equals_brute_force(name, umis, ks):
    """dcrx_umi_encode, the tile rule, the upper-triangle walk and the pair function together (tests/host_umi's plain loop
    over the kernel's iteration space) against the brute force, key for key.  k = 2^30 and 2^31 - 1 ask for every pair, as
    k = 24 does: 2 * k must not wrap."""
    L = _host_umi_lib()
    recs, tiles = nat.umi_encode(list(umis))
    recs, tiles = np.ascontiguousarray(recs), np.ascontiguousarray(tiles)
    for k in ks:
        want = cu.brute_keys(umis, k)
        if k in cu.K_HUGE:
            assert len(want) == len(umis) * (len(umis) - 1) // 2
        out = np.zeros(len(want) + 8, dtype=np.uint64)
        total = L.umi_host_walk(recs.ctypes.data, tiles.ctypes.data, len(tiles), k, out.ctypes.data, len(out))
        assert total == len(want), (k, total, len(want))
        got = np.sort(out[:total])
        assert (got == want).all(), k
        # too little room: the count is the same and nothing is written past it
        small = np.full(7 + 4, 0xDEAD, dtype=np.uint64)
        assert L.umi_host_walk(recs.ctypes.data, tiles.ctypes.data, len(tiles), k, small.ctypes.data, 7) == total
        assert (small[7:] == 0xDEAD).all()


def test_umi_limits_are_errors_not_aborts():
    with pytest.raises(nat.DcrxError) as e:
        nat.umi_encode(["A" * 25])
    assert e.value.code == -2 and "at most 24" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.umi_encode(["ACGTNSLX", "Q"])
    assert e.value.code == -2 and "distinct byte values" in str(e.value)
    with pytest.raises(nat.DcrxError) as e:
        nat.umi_neighbours_keys(["A" * 30, "A"], 2)
    assert e.value.code == -2
    with pytest.raises(ValueError):
        nat.umi_neighbours_keys(["AC", "AG"], -1)
    r = nat.lib().dcrx_umi_neighbours_device(None, None, 0, -1, None, 0, None, None)
    assert r == -1
    recs, tiles = nat.umi_encode([])
    assert len(recs) == 0 and len(tiles) == 0
