"""Several chains in one pass, through the HIP path: dcrx_decombine_chains against dcrx_decombine on each handle alone and
against the oracle, and the `-c a,b` stage on the TINY fixtures and on a batch of mixed read lengths."""
import json
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import pipeline, synth
from oracle import oracle as orc
from tests import chains_util as chu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu


def _tables(ts):
    return nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)


def _oracle(ts):
    vs, js = ts.half_splits
    return orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                            [r.upper() for r in ts.j_regions], vs, js)


def test_tiny_through_hip_path(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    fx = chu.tiny_workdir(tmp_path)
    pipeline.main(["decombine", "-in", "TINY_1.fq", "-c", "a,b", "-br", "R2", "-dz", "-dc", "-tfdir", "tags"])
    for name in ("alpha", "beta"):
        text = (tmp_path / f"dcr_TINY_1_{name}.n12").read_text()
        assert text == "".join(", ".join(r) + "\n" for r in fx[name]["reference_fixture_rows"])
        for k, v in fx[name]["counts_with_reconstructed_tagset"].items():
            assert dec.chain_counts[name[0]][k] == v, (name, k)


def test_tiny_pipeline_cluster_through_hip_path(tmp_path, monkeypatch):
    from decombinator_amd import translate
    monkeypatch.chdir(tmp_path)
    handed = {}
    monkeypatch.setattr(translate, "cdr3translator",
                        lambda inputargs, data=None: handed.setdefault(inputargs["chain"], []).extend(list(data)) or [])
    chu.tiny_workdir(tmp_path)
    pipeline.main(["pipeline", "-in", "TINY_1.fq", "-c", "a,b", "-br", "R2", "-dz", "-dc", "-tfdir", "tags", "-ol", "M13",
                   "--cluster"])
    want = json.load(open(os.path.join(chu.HERE, "golden", "tiny_freq.json")))
    for name in ("alpha", "beta"):
        assert (tmp_path / f"dcr_TINY_1_{name}.freq").read_text().splitlines() == want[name]
        assert [", ".join(map(str, r)) for r in handed[name[0]]] == want[name]
        assert (tmp_path / f"dcr_TINY_1_{name}.tsv").exists()


N_READS = 5_000_003          # more than two 2 M-read chunks, and an odd tail


@pytest.mark.parametrize("config", [3, 5])
def test_c_entry_equals_single_chain_entry(config):
    tagsets = synth.config3_tagsets() if config == 3 else synth.config5_tagsets()
    tables = [_tables(ts) for ts in tagsets]
    cfg = nat.synth_cfg(seed=1000 + config, sub_rate=0.02 if config == 5 else 0.005)
    half = N_READS // 2
    rng = np.random.default_rng(config)
    sample = np.sort(rng.choice(N_READS, size=1 << 16, replace=False))
    for pinned in (False, True):
        # reads drawn half from each chain's germlines (the first chain's, then the second's)
        parts = [nat.synth_reads_host(tables[0], cfg, 0, half, pinned=pinned),
                 nat.synth_reads_host(tables[1], cfg, half, N_READS - half, pinned=pinned)]
        stride = parts[0].stride
        packed = nat.pinned_empty((N_READS, stride), np.uint8) if pinned else np.empty((N_READS, stride), dtype=np.uint8)
        packed[:half] = parts[0].packed
        packed[half:] = parts[1].packed
        exc = [np.concatenate([parts[0].exc_read, parts[1].exc_read + np.uint32(half)]),
               np.concatenate([parts[0].exc_pos, parts[1].exc_pos]), np.concatenate([parts[0].exc_chr, parts[1].exc_chr])]
        del parts
        batch = nat.PackedBatch(packed, stride, cfg.read_len, None, *exc)
        assert batch.n_reads == N_READS and len(exc[0]) > 1000
        for orientation in ("reverse", "both"):
            got = nat.decombine_chains(tables, batch, orientation)
            for c, t in enumerate(tables):
                rec, cnt = nat.decombine(t, batch, orientation)
                pu.assert_records_equal(got[c][0], rec, what=f"config {config} chain {c} {orientation} pinned={pinned}")
                assert got[c][1].tobytes() == cnt.tobytes()
                assert int(cnt[nat.COUNTER_NAMES.index("vj_count")]) > N_READS // 10
                if not pinned and orientation == "reverse":
                    in_sample = np.isin(exc[0], sample)
                    sub = nat.PackedBatch(np.ascontiguousarray(packed[sample]), stride, cfg.read_len, None,
                                          np.searchsorted(sample, exc[0][in_sample]).astype(np.uint32),
                                          exc[1][in_sample].copy(), exc[2][in_sample].copy())
                    reads = nat.unpack_reads(sub)
                    orec, _ = pu.oracle_records(_oracle(tagsets[c]), reads, orientation, False, 130)
                    pu.assert_records_equal(got[c][0][sample], orec, reads, what=f"config {config} chain {c} vs oracle")
            one = nat.decombine_chains(tables[:1], batch, orientation)
            assert one[0][0].tobytes() == got[0][0].tobytes() and one[0][1].tobytes() == got[0][1].tobytes()


def test_mixed_read_lengths_through_the_stage(tmp_path, monkeypatch):
    """150 nt and 600 nt reads, two chains: the long reads leave each batch for a call of their own (the long form)."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 4096)
    ta, tb = synth.config3_tagsets()
    for ts in (ta, tb):
        ts.write(str(tmp_path / "tags"))
    chu.write_synth_pair(tmp_path, (ta, tb), 6000, seed=71, n_long=1500)
    got = chu.compare_with_single_runs(tmp_path, "a,b", ["-in", "SYN_1.fq", "-br", "R2", "-tfdir", "tags", "-dc", "-or", "both"])
    assert all(len(got[f"dcr_SYN_1_{c}.n12"]) > 10000 for c in ("alpha", "beta"))
