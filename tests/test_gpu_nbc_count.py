"""The barcode-free count through the HIP path: the count step (dcrx_decombine_count, dcrx_count_device) against a Counter
built on the host from dcrx_decombine's records, the chains entry against the single entry on each handle, and the
`-nbc --count-dcrs` stage on the TINY fixtures and on clonal synthetic reads."""
import collections
import functools

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import pipeline, synth
from tests import chains_util as chu
from tests import nbc_count_util as nu

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu", b"TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna")


def _tables(ts):
    return nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)


def _expected(rec, batch, first_index=0):
    """[(v, j, vdel, jdel, insert bytes, count, first ordinal)] in most_common() order, from records and their reads."""
    raw, off = nat.unpack_reads_raw(batch)
    raw = raw.tobytes()
    c, first = collections.Counter(), {}
    ok = np.nonzero(rec["status"] == 0)[0]
    v, j, vd, jd = (rec[f][ok].tolist() for f in ("v", "j", "vdel", "jdel"))
    s, l, fr = (rec[f][ok].tolist() for f in ("ins_start", "ins_len", "frame"))
    o0, o1 = off[ok].tolist(), off[ok + 1].tolist()
    for k, r in enumerate(ok.tolist()):
        if fr[k]:
            ins = raw[o0[k] + s[k]:o0[k] + s[k] + l[k]]
        else:
            e = o1[k] - s[k]
            ins = raw[e - l[k]:e][::-1].translate(_COMP)
        key = (v[k], j[k], vd[k], jd[k], ins)
        c[key] += 1
        if key not in first:
            first[key] = first_index + r
    return [k + (n, first[k]) for k, n in c.most_common()]


def _got(counted):
    t, off = counted["ins_text"], counted["ins_off"].tolist()
    cols = [counted[f].tolist() for f in ("v", "j", "vdel", "jdel", "count", "first")]
    return [(cols[0][k], cols[1][k], cols[2][k], cols[3][k], t[off[k]:off[k + 1]], cols[4][k], cols[5][k])
            for k in range(len(cols[0]))]


@pytest.mark.parametrize("orientation,pinned", [("reverse", False), ("forward", True), ("both", False)])
def test_count_step_nearly_distinct(orientation, pinned):
    ts = synth.config_tagset(2)
    t = _tables(ts)
    n = 5_000_000 + 12_345 if orientation == "reverse" else 2_500_017          # not a multiple of the 2 M chunk
    batch = nat.synth_reads_host(t, nat.synth_cfg(seed=41, n_rate=0.002), 0, n, pinned=pinned)
    rec, cnt = nat.decombine(t, batch, orientation)
    dc = nat.DcrCounts()
    cnt2 = nat.decombine_count(t, batch, dc, 1000, None, orientation)
    assert (cnt == cnt2).all()
    want = _expected(rec, batch, 1000)
    got = _got(dc.read())
    assert len(got) == len(want) and got == want
    assert sum(x[5] for x in got) == int(cnt[19])
    dc.close()


@pytest.mark.parametrize("orientation,pinned", [("reverse", True), ("both", False)])
def test_count_step_skewed(orientation, pinned):
    ts = synth.config_tagset(2)
    t = _tables(ts)
    reads = nu.clonal_reads(ts, 2_100_003, seed=43, n_pool=5000, zipf=1.1, orientation=orientation, exceptions=0.3, lower=0.2)
    batch = nat.pack_reads(reads)
    if pinned:
        p = nat.pinned_empty(batch.packed.shape, np.uint8)
        p[:] = batch.packed
        batch.packed = p
    rec, cnt = nat.decombine(t, batch, orientation)
    want = _expected(rec, batch)
    assert want[0][5] >= 0.1 * len(reads)          # the top clone holds at least a tenth of the reads
    dc = nat.DcrCounts()
    # two calls into one table: ordinals carry on, the table lasts across calls
    half = len(reads) // 2
    b1, b2 = nat.pack_reads(reads[:half]), nat.pack_reads(reads[half:])
    c1 = nat.decombine_count(t, b1, dc, 0, None, orientation)
    c2 = nat.decombine_count(t, b2, dc, half, None, orientation)
    assert (c1 + c2 == cnt).all()
    assert _got(dc.read()) == want
    dc.reset()
    nat.decombine_count(t, batch, dc, 0, None, orientation)
    assert _got(dc.read()) == want
    dc.close()


def test_count_device_with_index():
    """The device primitive with an index array: a batch split in two (the long-read split), ordinals from the index."""
    ts = synth.config_tagset(2)
    t = _tables(ts)
    reads = nu.clonal_reads(ts, 40_000, seed=45, n_pool=400, n_long=30, lower=0.3)
    whole = nat.pack_reads(reads)
    rec, _ = nat.decombine(t, whole)
    want = _expected(rec, whole, 7)
    is_long = np.array([len(r) > nat.FAST_MAX_READ_LEN for r in reads])
    dc = nat.DcrCounts()
    for idx in (np.nonzero(~is_long)[0], np.nonzero(is_long)[0]):
        part = nat.pack_reads([reads[i] for i in idx])
        db = nat.DeviceBatch.from_host(part)
        d_rec = nat.DeviceBuffer(16 * part.n_reads)
        d_cnt = nat.DeviceBuffer(8 * nat.N_COUNTERS)
        nat.decombine_device(t, db, d_rec, d_cnt)
        d_idx = nat.DeviceBuffer.from_host(idx.astype(np.uint32))
        nat.count_device(dc, d_rec, db, 7, d_idx)
        nat.synchronize()
    assert _got(dc.read()) == want
    dc.close()


@pytest.mark.parametrize("bits", [0, 3])
def test_colliding_hashes_stay_exact(bits):
    """Keys keep `bits` hash bits (dcrx_counts_set_hash_bits): distinct DCRs share hashes inside a batch (the stragglers of a
    run) and in the table (probing past a published slot of the same hash); the counts still equal the host Counter."""
    ts = synth.config_tagset(2)
    t = _tables(ts)
    reads = nu.clonal_reads(ts, 24_000 if bits else 8_000, seed=61 + bits, n_pool=500 if bits else 160, orientation="both",
                            exceptions=0.3, lower=0.3)
    batch = nat.pack_reads(reads)
    rec, _ = nat.decombine(t, batch, "both")
    want = _expected(rec, batch)
    assert len(want) > 50
    dc = nat.DcrCounts()
    dc.set_hash_bits(bits)
    half = len(reads) // 3
    nat.decombine_count(t, nat.pack_reads(reads[:half]), dc, 0, None, "both")
    nat.decombine_count(t, nat.pack_reads(reads[half:]), dc, half, None, "both")
    assert _got(dc.read()) == want
    with pytest.raises(nat.DcrxError, match="not empty"):
        dc.set_hash_bits(63)
    dc.reset()
    dc.set_hash_bits(63)
    nat.decombine_count(t, batch, dc, 0, None, "both")
    assert _got(dc.read()) == want
    dc.close()


@functools.lru_cache(maxsize=None)
def _edge_batch(n):
    """(tables, batch, expected table) of n reads drawn from 40 clonal reads in either orientation."""
    ts = synth.config_tagset(2)
    t = _tables(ts)
    batch = nat.pack_reads(nu.clonal_reads(ts, n, seed=71, n_pool=40, orientation="both"))
    rec, _ = nat.decombine(t, batch, "both")
    return t, batch, _expected(rec, batch)


@pytest.mark.parametrize("bits", [0, 3, 63])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_batches_on_a_block_edge(n, bits):
    """Batches that end on, one before and one behind a block of 256, and in a third block, of so few clones that runs of
    equal hashes lie across the blocks' edges (with no hash bits the batch is one run and every other DCR a straggler)."""
    t, batch, want = _edge_batch(n)
    assert len(want) > 10 and want[0][5] > 1
    dc = nat.DcrCounts()
    dc.set_hash_bits(bits)
    nat.decombine_count(t, batch, dc, 0, None, "both")
    assert _got(dc.read()) == want
    dc.close()


def test_chains_entry_equals_single_entry():
    ta, tb = synth.config3_tagsets()
    tables = [_tables(ta), _tables(tb)]
    reads = nu.clonal_reads(tb, 1_500_000, seed=47, n_pool=3000, exceptions=0.2) + \
        nu.clonal_reads(ta, 1_500_000, seed=48, n_pool=3000, lower=0.2)
    np.random.default_rng(1).shuffle(reads)
    batch = nat.pack_reads(reads)
    dcs = [nat.DcrCounts(), nat.DcrCounts()]
    cnts = nat.decombine_chains_count(tables, batch, dcs, 5)
    for t, dc, cnt in zip(tables, dcs, cnts):
        single = nat.DcrCounts()
        c1 = nat.decombine_count(t, batch, single, 5)
        assert (c1 == cnt).all()
        got = _got(dc.read())
        assert got == _got(single.read()) and len(got) > 100
        rec, _ = nat.decombine(t, batch)
        assert got == _expected(rec, batch, 5)
        single.close()


def test_stage_tiny_through_hip_path(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    fx = chu.tiny_workdir(tmp_path)
    pipeline.main(["decombine", "-in", "TINY_1.fq", "-c", "a,b", "-br", "R2", "-nbc", "--count-dcrs", "-dz", "-dc", "-tfdir", "tags"])
    for name in ("alpha", "beta"):
        want = collections.Counter(", ".join(r[:5]) for r in fx[name]["reference_fixture_rows"]).most_common()
        assert (tmp_path / f"dcr_TINY_1_{name}.nbc").read_text() == "".join(f"{k}, {n}\n" for k, n in want)
        for k, v in fx[name]["counts_with_reconstructed_tagset"].items():
            if k != "dcrfilter_barcodeN":
                assert dec.chain_counts[name[0]][k] == v, (name, k)


@pytest.mark.parametrize("case", ["both", "allow_ns_exceptions", "long_reads"])
def test_stage_synthetic_through_hip_path(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 4096)
    ts = synth.config_tagset(2)
    kw = {"both": dict(orientation="both", lower=0.3), "allow_ns_exceptions": dict(exceptions=0.5, lower=0.3, with_n=True),
          "long_reads": dict(n_long=25, lower=0.2, exceptions=0.2)}[case]
    reads = nu.clonal_reads(ts, 30_000, seed=51 + len(case), n_pool=2000, **kw)
    orientation = kw.get("orientation", "reverse")
    allow_ns = case == "allow_ns_exceptions"
    argv = nu.workdir_with(tmp_path, ts, reads) + ["-dz", "-or", orientation] + (["-N"] if allow_ns else [])
    pipeline.main(["decombine"] + argv)
    keys, cnt = nu.read_dcrs(nu.oracle_for(ts), reads, orientation, allow_ns)
    assert (tmp_path / "dcr_NBC_1_beta.nbc").read_text(encoding="latin-1") == nu.expected_nbc(keys)
    assert dec.counts["vj_count"] == sum(1 for k in keys if k)
