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
