"""Stage 2 of `collapse` (--cluster) on the CPU: grouping, the protoseq test, the components and the counting are libdcrx's
host code and Python; the UMI neighbour search (a HIP kernel) is replaced by an independent brute force here
(tests/collapse_cluster_util.py), the pattern of test_host_stage.py's _oracle_device.  Expected outputs come from the
reference's own collapsinator (tests/golden/collapse_cluster.json) and its TINY `.freq` files (tests/golden/tiny_freq.json)."""
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
