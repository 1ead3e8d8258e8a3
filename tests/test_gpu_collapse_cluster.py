"""Stage 2 of `collapse` (--cluster) on the MI355X: the UMI neighbour search kernel (dcrx_umi.hip) against an independent
CPU neighbour list, every fixture case of tests/golden/collapse_cluster.json through the real device path, and the TINY
FASTQ pair through `pipeline --cluster` to the reference's `.freq` files."""
import os
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from tests import collapse_cluster_util as cu
from tests import test_collapse_cluster as tcc

pytestmark = pytest.mark.gpu


def _umis(rng, n, alphabet="ACGT", n_rate=0.0):
    """Families of 12-nt-ish UMIs (substitutions and indels, so lengths vary), N bytes at n_rate."""
    out = []
    while len(out) < n:
        base = "".join(rng.choice(alphabet) for _ in range(rng.choice([11, 12, 12, 12, 13])))
        fam = [base]
        for _ in range(rng.choice([0, 0, 1, 2, 4])):
            s = list(rng.choice(fam))
            for _ in range(rng.randrange(1, 3)):
                op = rng.randrange(4)
                if op < 2:
                    s[rng.randrange(len(s))] = rng.choice(alphabet)
                elif op == 2 and len(s) < 24:
                    s.insert(rng.randrange(len(s) + 1), rng.choice(alphabet))
                elif len(s) > 1:
                    del s[rng.randrange(len(s))]
            fam.append("".join(s))
        for u in fam:
            if n_rate and rng.random() < n_rate:
                i = rng.randrange(len(u))
                u = u[:i] + "N" + u[i + 1:]
            out.append(u)
    return list(dict.fromkeys(out))[:n]          # distinct, as the groups' UMIs are


@pytest.mark.parametrize("n,k", [(50000, 1), (50000, 2), (20000, 3), (200000, 1)])
def test_kernel_pairs_equal_cpu_neighbours(n, k):
    rng = random.Random(n + k)
    umis = _umis(rng, n, n_rate=0.02)
    keys = nat.umi_neighbours_keys(umis, k)
    r, c = cu.symdel_neighbours(umis, k)
    want = (r.astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64)
    assert len(keys) == len(want)
    assert (keys == want).all()


def test_kernel_capacity_overflow_and_retry():
    rng = random.Random(3)
    umis = _umis(rng, 20000)
    want = nat.umi_neighbours_keys(umis, 2)
    assert len(want) > 10
    got = nat.umi_neighbours_keys(umis, 2, cap=7)           # first call too small: repeated with room for all
    assert (got == want).all()
    text, off = nat.text_and_offsets(umis)
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(7, dtype=np.uint64)
    total = nat.check(nat.lib().dcrx_umi_neighbours(buf.ctypes.data, off.ctypes.data, len(umis), 2, out.ctypes.data, 7))
    assert total == len(want)


def test_kernel_small_inputs():
    assert len(nat.umi_neighbours_keys([], 2)) == 0
    assert len(nat.umi_neighbours_keys(["ACGTACGTACGT"], 2)) == 0
    assert len(nat.umi_neighbours_keys(["AAAAAAAAAAAA", "CCCCCCCCCCCC", "GGGGGGGGGGGG"], 2)) == 0
    keys = nat.umi_neighbours_keys(["AC", "ACGTACGTACGTACGTACGTACGT", "A", ""], 30)   # k beyond every length: all pairs
    assert keys.tolist() == [(i << 32) | j for i in range(4) for j in range(i + 1, 4)]


# ---- constructed lists (collapse_cluster_util): each compared in full with the brute force ----

def _check_keys(umis, k, **kw):
    want = cu.brute_keys(umis, k)
    got = nat.umi_neighbours_keys(list(umis), k, **kw)
    assert len(got) == len(want), (k, len(got), len(want))
    assert (got == want).all()
    return want


@pytest.mark.parametrize("k", [24, 2 ** 30, 2 ** 31 - 1])
def test_all_pairs_full_ballots(k):
    """Every pair is a hit: 64-lane ballots, four waves of a diagonal tile, three tiles, and more pairs than the first
    call's room.  A k far beyond every length asks for the same pairs."""
    umis = cu.umi_all_pairs_list()
    assert len(umis) == 600 and "" in umis and len(set(umis)) == 600 and set("".join(umis)) == set(cu.UMI_SYMBOLS)
    assert {len(u) for u in umis} == set(range(25))
    want = _check_keys(umis, k)
    assert len(want) == 600 * 599 // 2 == 179700 > 4 * 600 + 1024


@pytest.mark.parametrize("k,n_pairs", [(2, 14196), (1, 168 + 24 * 21)])
def test_one_substitution_ball(k, n_pairs):
    umis = cu.umi_ball_list()
    assert len(set(umis)) == 169 and {len(u) for u in umis} == {24} and set("".join(umis)) == set(cu.UMI_SYMBOLS)
    assert len(_check_keys(umis, k)) == n_pairs


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_families_with_repeats_and_length_limits(k):
    umis = cu.umi_family_list()
    assert len(umis) == 1300 and {0, 1, 2, 11, 12, 13, 23, 24} <= {len(u) for u in umis} and "N" in "".join(umis)
    want = _check_keys(umis, k)
    if k == 0:                                    # exactly the repeated strings
        by_text = {}
        for i, u in enumerate(umis):
            by_text.setdefault(u, []).append(i)
        repeats = sorted((a << 32) | b for g in by_text.values() for x, a in enumerate(g) for b in g[x + 1:])
        assert want.tolist() == repeats
        assert 0 < len(want) < len(cu.brute_keys(umis, 1))


@pytest.mark.parametrize("n", cu.TILE_EDGE_N)
def test_tile_edges(n):
    umis = cu.umi_family_list(n, cu.TILE_EDGE_SEED)
    assert len(umis) == n
    want = _check_keys(umis, 2)
    if n % 256 == 1:                              # the last tile holds one record, and an expected pair ends in it
        recs, tiles = nat.umi_encode(list(umis))
        assert tiles[-1, 6] == 1
        alone = int(recs[(len(tiles) - 1) * 256, 14])
        assert ((want >> np.uint64(32)) == alone).any() or ((want & np.uint64(0xFFFFFFFF)) == alone).any()


@pytest.mark.parametrize("k", [1, 2])
def test_tiles_exactly_at_reach_by_length(k):
    umis = cu.umi_reach_len_list(k)
    tcc._reach_len_layout(umis, k)
    _check_keys(umis, k)


@pytest.mark.parametrize("k", [1, 2])
def test_tiles_exactly_at_reach_by_composition(k):
    umis = cu.umi_reach_comp_list(k)
    tcc._reach_comp_layout(umis, k)
    _check_keys(umis, k)


SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.mark.parametrize("cap", [0, 7, 14196, None], ids=["cap0", "cap7", "cap14196", "null"])
def test_neighbours_device_on_a_stream_of_the_callers_with_too_little_room(cap):
    """dcrx_umi_neighbours_device on a stream of the caller's: *d_total is the number found whatever the room, the first
    min(cap, total) words are distinct expected keys, nothing is written from word `cap` on, and a second call on the same
    buffers counts from zero again.  cap None: pair_cap = 0 with a null d_pairs.  The buffer has room for every pair and 64
    words more, all holding a sentinel; the words checked are all of those from `cap` on, the 64 past it among them."""
    umis = cu.umi_ball_list()
    want = cu.brute_keys(umis, 2)
    total = len(want)
    assert total == 14196
    recs, tiles = nat.umi_encode(list(umis))
    d_recs, d_tiles = nat.DeviceBuffer.from_host(recs), nat.DeviceBuffer.from_host(tiles)
    d_total = nat.DeviceBuffer.from_host(np.full(1, 12345, dtype=np.uint64))            # not zero: the call zeroes it
    room = total + 64
    d_pairs = nat.DeviceBuffer.from_host(np.full(room, SENTINEL, dtype=np.uint64))
    s = nat.Stream()
    for _ in range(2):
        nat.check(nat.lib().dcrx_umi_neighbours_device(d_recs.ptr, d_tiles.ptr, len(tiles), 2, None if cap is None else d_pairs.ptr,
                                                       cap or 0, d_total.ptr, s.ptr))
        s.synchronize()
        assert int(d_total.to_host(np.uint64, 1)[0]) == total
        words = d_pairs.to_host(np.uint64, room)
        n_written = min(cap or 0, total)
        assert (words[n_written:] == SENTINEL).all()
        got = words[:n_written]
        assert len(np.unique(got)) == n_written and np.isin(got, want).all()


@pytest.mark.parametrize("case", cu.cases(), ids=[c["params"]["name"] for c in cu.cases()])
def test_fixture_case_on_device(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cu.check_case(case, cu.run_case(case, tmp_path, via_cli=True))


@pytest.mark.parametrize("chain_name", ["alpha", "beta"])
def test_tiny_fastq_pipeline_cluster_equals_reference_freq(chain_name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    want, handed = tcc.tiny_pipeline(chain_name, tmp_path, monkeypatch)
    assert (tmp_path / f"dcr_TINY_1_{chain_name}.freq").read_text().splitlines() == want
    assert [", ".join(map(str, r)) for r in handed] == want
    assert os.path.exists(tmp_path / f"dcr_TINY_1_{chain_name}.n12")
