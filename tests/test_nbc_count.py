"""The barcode-free count (`decombine -nbc --count-dcrs`) on the CPU: the oracle stands in for nat.count_dcrs and
nat.DcrCounts (the pattern of test_chains.py), libdcrx's host formatter writes the `.nbc`.  Expectations come from the
reference's own TINY rows and from the oracle's per-read DCRs fed to a collections.Counter."""
import collections
import gzip
import json
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import io as dio
from decombinator_amd import pipeline, sharded, synth
from tests import chains_util as chu
from tests import nbc_count_util as nu


@pytest.fixture()
def oracle_count(monkeypatch):
    return nu.OracleCountDevice(monkeypatch)


def _tiny_argv(chain):
    return ["decombine", "-in", "TINY_1.fq", "-c", chain, "-br", "R2", "-nbc", "--count-dcrs", "-dz", "-dc", "-tfdir", "tags"]


@pytest.mark.parametrize("name,n_rows,n_distinct", [("beta", 48, 43), ("alpha", 35, 31)])
def test_tiny_counts_equal_reference_rows(name, n_rows, n_distinct, tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    fx = chu.tiny_workdir(tmp_path)
    pipeline.main(_tiny_argv(name[0]))
    rows = fx[name]["reference_fixture_rows"]
    assert len(rows) == n_rows
    want = collections.Counter(", ".join(r[:5]) for r in rows).most_common()
    assert len(want) == n_distinct
    text = (tmp_path / f"dcr_TINY_1_{name}.nbc").read_text()
    assert text == "".join(f"{k}, {n}\n" for k, n in want)
    if name == "beta":
        assert want[0][1] == 3 and [n for _, n in want].count(2) >= 2
    else:
        assert any(k.endswith(", ") for k, _ in want)          # an empty insert: "v, j, vdel, jdel, , n"
        assert any(", , " in ln for ln in text.splitlines())
    for k, v in fx[name]["counts_with_reconstructed_tagset"].items():
        if k != "dcrfilter_barcodeN":
            assert dec.counts[k] == v, k
    assert dec.counts["dcrfilter_barcodeN"] == 0
    assert len(oracle_count.calls) == 1 and oracle_count.calls[0][:3] == (dec.counts["read_count"], 1, 0)
    assert not os.path.exists(tmp_path / f"dcr_TINY_1_{name}.n12")
    logs = list((tmp_path / "Logs").glob("*_Decombinator_Summary.csv"))
    assert len(logs) == 1
    log = logs[0].read_text()
    assert f"NumberReadsInput,{dec.counts['read_count']}" in log and f"NumberReadsDecombined,{n_rows}" in log


def test_tiny_decombinator_returns_rows(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    fx = chu.tiny_workdir(tmp_path)
    args = dio.create_args_dict(infile="TINY_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", nobarcoding=True,
                                count_dcrs=True, dontcount=True)
    rows = dec.decombinator(args)
    want = collections.Counter(", ".join(r[:5]) for r in fx["beta"]["reference_fixture_rows"]).most_common()
    assert [", ".join(r[:5]) for r in rows] == [k for k, _ in want]
    assert [r[5] for r in rows] == [n for _, n in want]
    assert all(len(r) == 6 for r in rows)


def test_tiny_both_chains_equal_single_runs(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    got = chu.compare_with_single_runs(tmp_path, "a,b", ["-in", "TINY_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "-dz", "-dc",
                                                         "-tfdir", "tags"])
    assert sorted(k for k in got if not k.startswith("Logs")) == ["dcr_TINY_1_alpha.nbc", "dcr_TINY_1_beta.nbc"]
    # the list run: one call per batch for both chains
    assert oracle_count.calls[0][1] == 2


@pytest.mark.parametrize("case", ["both", "allow_ns_exceptions", "long_reads", "lower_no_n"])
def test_synthetic_counts(case, tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 64)          # many batches: copies of one DCR on both sides of a boundary
    ts = synth.config_tagset(2)
    kw = {"both": dict(orientation="both"), "allow_ns_exceptions": dict(exceptions=0.5, lower=0.3, with_n=True),
          "long_reads": dict(n_long=20, lower=0.2), "lower_no_n": dict(exceptions=0.4, lower=0.4, orientation="forward")}[case]
    reads = nu.clonal_reads(ts, 900, seed=7 + len(case), **kw)
    argv = nu.workdir_with(tmp_path, ts, reads) + ["-dz"]
    orientation = kw.get("orientation", "reverse")
    allow_ns = case == "allow_ns_exceptions"
    argv += ["-or", orientation] + (["-N"] if allow_ns else [])
    pipeline.main(["decombine"] + argv)
    keys, cnt = nu.read_dcrs(nu.oracle_for(ts), reads, orientation, allow_ns)
    text = (tmp_path / "dcr_NBC_1_beta.nbc").read_text(encoding="latin-1")
    assert text == nu.expected_nbc(keys)
    # the DCRs repeat, across batch boundaries too
    first_batch = set(k for k in keys[:64] if k)
    assert any(k in first_batch for k in keys[64:] if k)
    assert collections.Counter(k for k in keys if k).most_common(1)[0][1] >= 20
    if case == "allow_ns_exceptions":
        assert any(any(c not in "ACGT" for c in ln.split(", ")[4]) for ln in text.splitlines())
    if case == "lower_no_n":
        assert any(any(c.islower() for c in ln.split(", ")[4]) for ln in text.splitlines())
    if case == "long_reads":
        assert any(index for (_, _, _, index) in oracle_count.calls)
        assert any(len(r) > 511 and k for r, k in zip(reads, keys))
    assert dec.counts["read_count"] == len(reads)
    assert dec.counts["vj_count"] == sum(1 for k in keys if k)
    assert dec.counts["dcrfilter_barcodeN"] == 0


def test_fasta_records_are_reads(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    ts = synth.config_tagset(2)
    reads = nu.clonal_reads(ts, 200, seed=3)
    argv = nu.workdir_with(tmp_path, ts, reads, fasta=True) + ["-dz"]
    pipeline.main(["decombine"] + argv)          # (no -dk: the FASTQ check does not apply to a FASTA input of the count)
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads)
    assert (tmp_path / "dcr_NBC_1_beta.nbc").read_text() == nu.expected_nbc(keys)
    # a FASTQ input is still checked
    (tmp_path / "BAD_1.fq").write_text("@r0\nACGT\n+\nII\n@r1\nACGT\n+\nII\n")
    with pytest.raises(ValueError, match="Length of read"):
        pipeline.main(["decombine"] + argv[:1] + ["BAD_1.fq"] + argv[2:])


def test_gzip_plain_and_extension(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    ts = synth.config_tagset(2)
    reads = nu.clonal_reads(ts, 300, seed=11)
    argv = nu.workdir_with(tmp_path, ts, reads)
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads)
    want = nu.expected_nbc(keys)
    for d, extra, name in (("gz", [], "dcr_NBC_1_beta.nbc.gz"), ("plain", ["-dz"], "dcr_NBC_1_beta.nbc"),
                           ("ext", ["-dz", "-ex", "dcrs"], "dcr_NBC_1_beta.dcrs"), ("pf", ["-pf", "x_"], "x_NBC_1_beta.nbc.gz")):
        (tmp_path / d).mkdir()
        pipeline.main(["decombine"] + argv + ["-op", f"{d}/"] + extra)
        assert sorted(x for x in os.listdir(tmp_path / d) if x != "Logs") == [name]
        p = tmp_path / d / name
        got = gzip.open(p).read() if name.endswith(".gz") else p.read_bytes()
        assert got.decode() == want
        assert oct(os.stat(p).st_mode)[-3:] == "666"
    # the gzip input reads the same
    with open(tmp_path / "NBC_1.fq", "rb") as f, gzip.open(tmp_path / "GZ_1.fq.gz", "wb") as g:
        g.write(f.read())
    (tmp_path / "gzin").mkdir()
    pipeline.main(["decombine"] + argv[:1] + ["GZ_1.fq.gz"] + argv[2:] + ["-op", "gzin/", "-dz"])
    assert (tmp_path / "gzin" / "dcr_GZ_1_beta.nbc").read_text() == want


def _translate_stubs(monkeypatch):
    """The synthetic tag sets carry no translate gene tables: the gene import and the CDR3 call are stood in for, the rest of
    cdr3translator (the rows' fields, duplicate_count, av_UMI_cluster_size) runs as it is."""
    from decombinator_amd import translate
    monkeypatch.setattr(translate, "import_gene_information", lambda inputargs: None)
    monkeypatch.setattr(translate, "set_gene_information", lambda g: None)

    def cdr3_batch(rows, headers, inputargs):
        out = []
        for r in rows:
            rec = {h: "" for h in headers}
            rec.update(productive="T", sequence="|".join(str(x).strip() for x in r[:5]))
            out.append(rec)
        return out
    monkeypatch.setattr(translate, "cdr3_batch", cdr3_batch)
    return translate


def _tsv_rows(path):
    text = (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)).read().splitlines()
    head = text[0].split("\t")
    return [dict(zip(head, ln.split("\t"))) for ln in text[1:]]


def test_pipeline_writes_nbc_and_tsv(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    translate = _translate_stubs(monkeypatch)
    from decombinator_amd import collapse
    monkeypatch.setattr(collapse, "collapsinator", lambda *a, **k: pytest.fail("collapse ran"))
    ts = synth.config_tagset(2)
    reads = nu.clonal_reads(ts, 400, seed=21)
    pipeline.main(["pipeline"] + nu.workdir_with(tmp_path, ts, reads) + ["-dz"])
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads)
    want = collections.Counter(k for k in keys if k).most_common()
    assert (tmp_path / "dcr_NBC_1_beta.nbc").read_text() == nu.expected_nbc(keys)
    rows = _tsv_rows(tmp_path / "dcr_NBC_1_beta.tsv")
    assert [int(r["duplicate_count"]) for r in rows] == [n for _, n in want]
    assert [r["sequence"] for r in rows] == [k.replace(", ", "|") for k, _ in want]
    assert all(r["av_UMI_cluster_size"] == "" for r in rows)
    assert translate.counts["line_count"] == len(want)
    assert not os.path.exists(tmp_path / "dcr_NBC_1_beta.n12")


def test_translate_reads_nbc_gz(tmp_path, monkeypatch, oracle_count):
    monkeypatch.chdir(tmp_path)
    ts = synth.config_tagset(2)
    reads = nu.clonal_reads(ts, 300, seed=23)
    pipeline.main(["decombine"] + nu.workdir_with(tmp_path, ts, reads))
    _translate_stubs(monkeypatch)
    pipeline.main(["translate", "-in", "dcr_NBC_1_beta.nbc.gz", "-c", "b", "-nbc", "--count-dcrs", "-dz", "-tfdir", "tags"])
    keys, _ = nu.read_dcrs(nu.oracle_for(ts), reads)
    want = collections.Counter(k for k in keys if k).most_common()
    rows = _tsv_rows(tmp_path / "dcr_NBC_1_beta.tsv")
    assert [int(r["duplicate_count"]) for r in rows] == [n for _, n in want]
    assert all(r["av_UMI_cluster_size"] == "" for r in rows)
    # without --count-dcrs the six-field rows are what they always were to translate: a seventh field is parsed
    with pytest.raises(IndexError):
        pipeline.main(["translate", "-in", "dcr_NBC_1_beta.nbc.gz", "-c", "b", "-dz", "-tfdir", "tags"])


def test_refusals_before_anything_is_read(tmp_path, monkeypatch, oracle_count, capsys):
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    base = ["-in", "TINY_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "--count-dcrs"]
    for argv, msg in ((["decombine"] + base, "needs -nbc"),
                      (["pipeline"] + base, "needs -nbc"),
                      (["pipeline"] + base + ["-nbc", "--cluster"], "--cluster"),
                      (["decombine"] + base + ["-nbc", "-sa"], "-sa"),
                      (["pipeline"] + base + ["-nbc", "-sa"], "-sa"),
                      (["collapse", "-in", "dcr_TINY_1_beta.n12", "-c", "b", "-nbc", "--count-dcrs"], "collapse"),
                      (["translate", "-in", "dcr_TINY_1_beta.nbc", "-c", "b", "--count-dcrs"], "needs -nbc")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
        assert msg in capsys.readouterr().err, argv
    args = dio.create_args_dict(infile="TINY_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", count_dcrs=True)
    with pytest.raises(ValueError, match="needs -nbc"):
        dec.decombinator(dict(args))
    with pytest.raises(ValueError, match="--cluster"):
        dec.decombinator(dict(args, nobarcoding=True, cluster=True))
    with pytest.raises(ValueError, match="-sa"):
        dec.decombinator_chains(dict(args, chain="a,b", nobarcoding=True, sampling_analysis=True))
    with pytest.raises(ValueError, match="sharded"):
        sharded.decombinator_sharded(dict(args, nobarcoding=True), comm=None)
    with pytest.raises(ValueError, match="sharded"):
        dec.decombinator(dict(args, nobarcoding=True), shard=(0, 2))
    assert not os.path.exists(tmp_path / "Logs") or not any("Summary" in x for x in os.listdir(tmp_path / "Logs"))


def test_nbc_alone_unchanged(tmp_path, monkeypatch, oracle_count):
    """-nbc without --count-dcrs writes what it wrote before: an empty `.n12` (the read loop never runs)."""
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    assert dio.create_args_dict(infile="x", chain="b", bc_read="R2")["count_dcrs"] is False
    assert dio.cli_args(["decombine", "-in", "x_1.fq", "-br", "R2", "-nbc"])["count_dcrs"] is False
    pipeline.main(["decombine", "-in", "TINY_1.fq", "-c", "b", "-br", "R2", "-nbc", "-dz", "-dc", "-s", "-tfdir", "tags"])
    assert (tmp_path / "dcr_TINY_1_beta.n12").read_text() == ""
    assert sorted(os.listdir(tmp_path)) == sorted(["TINY_1.fq", "TINY_2.fq", "tags", "dcr_TINY_1_beta.n12"])
    assert oracle_count.calls == [] and dec.counts["read_count"] == 0


def test_format_counts_matches_python():
    rng = np.random.default_rng(5)
    n = 500
    ins = ["".join(rng.choice(list("ACGTNacgtRY"), size=int(rng.integers(0, 40)))) for _ in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in ins])
    c = {"v": rng.integers(0, 65535, n).astype(np.uint16), "j": rng.integers(0, 65535, n).astype(np.uint16),
         "vdel": rng.integers(0, 255, n).astype(np.uint8), "jdel": rng.integers(0, 255, n).astype(np.uint8),
         "count": rng.integers(1, 1 << 62, n, dtype=np.int64).astype(np.uint64), "first": np.arange(n, dtype=np.uint64),
         "ins_off": off, "ins_text": "".join(ins).encode()}
    want = "".join(f"{c['v'][k]}, {c['j'][k]}, {c['vdel'][k]}, {c['jdel'][k]}, {ins[k]}, {c['count'][k]}\n" for k in range(n))
    assert nat.format_counts(c).decode() == want
    assert nat.format_counts(c, ",").decode() == want.replace(", ", ",")
    assert [r[:5] + [r[5]] for r in nat.count_rows(c)][:3] == [[str(c["v"][k]), str(c["j"][k]), str(c["vdel"][k]),
                                                               str(c["jdel"][k]), ins[k], int(c["count"][k])] for k in range(3)]
    empty = {k: v[:0] for k, v in c.items() if k != "ins_off"}
    empty.update(ins_off=np.zeros(1, np.uint64), ins_text=b"")
    assert nat.format_counts(empty) == b""


def test_count_entry_argument_errors():
    fx = json.load(open(os.path.join(chu.HERE, "golden", "tiny_beta.json")))["tagset"]
    t = nat.Tables(fx["v_tags"], fx["v_jumps"], fx["v_regions"], fx["j_tags"], fx["j_jumps"], fx["j_regions"], 10, 6)
    b = nat.pack_reads(["ACGT" * 10])
    cfg = nat.make_cfg()
    cnt = np.zeros(nat.N_COUNTERS, np.uint64)
    import ctypes as C
    rc = nat.lib().dcrx_decombine_count(t.handle, C.byref(cfg), C.byref(b.as_c()), None, 0, None, cnt.ctypes.data)
    assert rc == -1 and "counts is null" in nat.lib().dcrx_last_error().decode()
    dc = nat.DcrCounts()           # (nothing touches the device before the first step)
    assert nat.count_rows(dc.read()) == []
    t2 = nat.Tables(fx["v_tags"], fx["v_jumps"], fx["v_regions"], fx["j_tags"], fx["j_jumps"], fx["j_regions"], 10, 6)
    h = (C.c_void_p * 2)(t.handle, t2.handle)
    ch = (C.c_void_p * 2)(dc.handle, dc.handle)
    cp = (C.c_void_p * 2)(cnt.ctypes.data, cnt.ctypes.data)
    assert nat.lib().dcrx_decombine_chains_count(h, 2, C.byref(cfg), C.byref(b.as_c()), ch, 0, None, cp) == -1
    assert "same counts handle twice" in nat.lib().dcrx_last_error().decode()
    ch = (C.c_void_p * 2)(dc.handle, None)
    assert nat.lib().dcrx_decombine_chains_count(h, 2, C.byref(cfg), C.byref(b.as_c()), ch, 0, None, cp) == -1
    assert "counts[c] is null" in nat.lib().dcrx_last_error().decode()
    with pytest.raises(nat.DcrxError, match="0 .. 63"):
        dc.set_hash_bits(64)
    dc.set_hash_bits(5)            # (an empty table takes it)
    dc.close()


def _host_count_lib():
    import ctypes as C
    import subprocess
    d = os.path.join(chu.HERE, "host_count")
    subprocess.check_call(["make", "-s", "-C", d])
    L = C.CDLL(os.path.join(d, "build", "libcount_host.so"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.count_host_insert.restype = None
    L.count_host_insert.argtypes = [vp, u32, u32, u32, u32, vp, vp, u32, vp]
    L.count_host_header.restype = u64
    L.count_host_header.argtypes = [u32, u32, u32, u32, u32]
    L.count_host_hash.restype = u64
    L.count_host_hash.argtypes = [u64, vp, u32]
    L.count_host_equal.restype = C.c_int
    L.count_host_equal.argtypes = [u64, vp, u64, vp]
    return L


def test_per_key_code_on_host_matches_python():
    """The kernels' key code (dcrx_count_core.h built by g++) against Python on random reads with exception bytes: the insert
    is the frame read's slice (revcomp() in the reverse frame), equal keys hash equal, and only equal keys compare equal."""
    L = _host_count_lib()
    rng = np.random.default_rng(17)
    alphabet = list("ACGT" * 6 + "NacgtnRYKMSWBDHVryk.-")
    keys = []
    for it in range(3000):
        n = int(rng.integers(1, 300))
        read = "".join(rng.choice(alphabet, size=n))
        b = nat.pack_reads([read])
        exc = [(int(p), int(c)) for r, p, c in zip(b.exc_read, b.exc_pos, b.exc_chr) if r == 0]
        ep = np.array([p for p, _ in exc] or [0], np.uint16)
        ec = np.array([c for _, c in exc] or [0], np.uint8)
        frame = int(rng.integers(0, 2))
        s = int(rng.integers(0, n))
        ln = int(rng.integers(0, n - s + 1))
        out = np.zeros(max(1, ln), np.uint8)
        L.count_host_insert(b.packed.ctypes.data, n, frame, s, ln, ep.ctypes.data, ec.ctypes.data, len(exc), out.ctypes.data)
        frame_read = read if frame else dec.revcomp(read)
        ins = frame_read[s:s + ln]
        assert out[:ln].tobytes().decode("latin-1") == ins, (read, frame, s, ln)
        v, j, vd, jd = (int(x) for x in rng.integers(0, 3, size=4))
        keys.append(((v, j, vd, jd, ins), L.count_host_header(v, j, vd, jd, ln), out[:ln].copy()))
    # a few keys that differ from another only in case or in one exception byte
    for k in range(50):
        (v, j, vd, jd, ins), hdr, buf = keys[k]
        if ins:
            b2 = buf.copy()
            b2[0] = ord(ins[0].swapcase()) if ins[0].isalpha() else ord("N")
            keys.append(((v, j, vd, jd, b2.tobytes().decode("latin-1")), hdr, b2))
    for a in range(0, len(keys), 7):
        for b_ in (a, (a * 31 + 5) % len(keys), min(len(keys) - 1, a + 3000)):
            ka, ha, ba = keys[a]
            kb, hb, bb = keys[b_]
            eq = L.count_host_equal(ha, ba.ctypes.data, hb, bb.ctypes.data)
            assert eq == (ka == kb), (ka, kb)
            if ka == kb:
                assert L.count_host_hash(ha, ba.ctypes.data, len(ka[4])) == L.count_host_hash(hb, bb.ctypes.data, len(kb[4]))
    hashes = [L.count_host_hash(h, b.ctypes.data, len(k[4])) for k, h, b in keys]
    assert all(x < (1 << 63) for x in hashes)                        # NO_KEY (all ones) is never a key's hash
    distinct = {k: x for (k, _, _), x in zip(keys, hashes)}
    assert len(set(distinct.values())) == len(distinct)              # (no collision on these few thousand keys)
