"""Several chains in one pass over the FASTQ (`-c a,b`), on the CPU: the oracle stands in for nat.decombine_chains (and
nat.decombine, for the single-chain runs the list run is compared with), the pattern of test_host_stage.py.  The list run
must write, per chain, exactly what a run with that chain alone writes; the C entry's argument errors come back as codes."""
import ctypes as C
import json
import os

import pytest

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import io as dio
from decombinator_amd import pipeline, sharded, synth
from tests import chains_util as chu
from tests import collapse_cluster_util as cu


@pytest.fixture()
def oracle_device(monkeypatch):
    return chu.OracleDevice(monkeypatch)


def _tiny_argv():
    return ["-in", "TINY_1.fq", "-br", "R2", "-dz", "-dc", "-tfdir", "tags"]


def test_tiny_both_chains_one_pass(tmp_path, monkeypatch, oracle_device):
    monkeypatch.chdir(tmp_path)
    fx = chu.tiny_workdir(tmp_path)
    (tmp_path / "multi").mkdir()
    pipeline.main(["decombine", "-c", "a,b", "-op", "multi/"] + _tiny_argv())
    for name, n_rows in (("alpha", 35), ("beta", 48)):
        want = fx[name]["reference_fixture_rows"]
        assert len(want) == n_rows
        text = (tmp_path / "multi" / f"dcr_TINY_1_{name}.n12").read_text()
        assert text == "".join(", ".join(r) + "\n" for r in want)
        got = dec.chain_counts[name[0]]
        for k, v in fx[name]["counts_with_reconstructed_tagset"].items():
            assert got[k] == v, (name, k)
    assert oracle_device.single_calls == 0 and len(oracle_device.chains_calls) == 1
    # the two summary logs: line for line those of the single-chain runs (apart from the time lines)
    for name in ("alpha", "beta"):
        d = tmp_path / f"single_{name}"
        d.mkdir()
        pipeline.main(["decombine", "-c", name[0], "-op", f"single_{name}/"] + _tiny_argv())
        logs = list((d / "Logs").glob("*.csv"))
        assert len(logs) == 1 and f"_{name}_TINY_1_" in logs[0].name
        assert chu.log_lines(logs[0]) == chu.log_lines(tmp_path / "multi" / "Logs" / logs[0].name)


def test_tiny_pipeline_cluster_both_chains(tmp_path, monkeypatch, oracle_device):
    from decombinator_amd import translate
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(nat, "umi_neighbours", cu.brute_neighbours)
    handed = {}
    # the reconstructed tag sets carry no translate gene tables: a stand-in records what each chain's call was handed
    monkeypatch.setattr(translate, "cdr3translator",
                        lambda inputargs, data=None: handed.setdefault(inputargs["chain"], []).extend(list(data)) or [])
    chu.tiny_workdir(tmp_path)
    pipeline.main(["pipeline", "-c", "a,b", "-ol", "M13", "--cluster"] + _tiny_argv())
    want = json.load(open(os.path.join(chu.HERE, "golden", "tiny_freq.json")))
    for name in ("alpha", "beta"):
        assert (tmp_path / f"dcr_TINY_1_{name}.freq").read_text().splitlines() == want[name]
        assert [", ".join(map(str, r)) for r in handed[name[0]]] == want[name]
        assert (tmp_path / f"dcr_TINY_1_{name}.n12").exists() and (tmp_path / f"dcr_TINY_1_{name}.tsv").exists()
    assert sorted(handed) == ["a", "b"]
    summaries = [x for x in os.listdir(tmp_path / "Logs") if "Collapsing_Summary" in x]
    assert any("_alpha_" in x for x in summaries) and any("_beta_" in x for x in summaries)


def test_one_pass_asserted(tmp_path, monkeypatch, oracle_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 64)
    opened = []
    real_reader = nat.FastqReader

    class CountingReader(real_reader):
        def __init__(self, path, *a, **k):
            opened.append(path)
            super().__init__(path, *a, **k)
    monkeypatch.setattr(nat, "FastqReader", CountingReader)
    chu.tiny_workdir(tmp_path)
    args = dio.create_args_dict(infile="TINY_1.fq", chain="a,b", bc_read="R2", dontgzip=True, dontcount=True,
                                tagfastadir="tags", outpath="", command="decombine")
    out = dec.decombinator_chains(args)
    assert list(out) == ["a", "b"] and (len(out["a"]), len(out["b"])) == (35, 48)
    assert sorted(opened) == ["TINY_1.fq", "TINY_2.fq"]                 # one reader per file
    assert oracle_device.chains_calls == [64, 42]                       # one device call per batch of 106 reads
    assert oracle_device.single_calls == 0
    assert args["chain"] == "a,b"                                       # the caller's arguments are left alone
    assert dec.stage_seconds.keys() >= {"read", "pack", "device", "rows", "rows:a", "rows:b", "close"}


@pytest.mark.parametrize("chains,flags", [
    ("a,b", ["-or", "both"]),
    ("b,a", ["-N", "-sa"]),
    ("a,b", ["-sa", "-ln", "60"]),
], ids=["both-orientations", "allowNs-sampling", "sampling-lenthreshold"])
def test_synthetic_alpha_beta_equals_single_runs(chains, flags, tmp_path, monkeypatch, oracle_device):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 256)
    ta, tb = synth.config3_tagsets()
    for ts in (ta, tb):
        ts.write(str(tmp_path / "tags"))
    chu.write_synth_pair(tmp_path, (ta, tb), 600, seed=31, n_long=7)
    got = chu.compare_with_single_runs(tmp_path, chains, ["-in", "SYN_1.fq", "-br", "R2", "-tfdir", "tags", "-dc"] + flags)
    assert {"dcr_SYN_1_alpha.n12", "dcr_SYN_1_beta.n12"} <= set(got)
    assert all(len(got[f"dcr_SYN_1_{c}.n12"]) > 1000 for c in ("alpha", "beta"))


def test_synthetic_gamma_delta_r1_mode_equals_single_runs(tmp_path, monkeypatch, oracle_device):
    """Mouse gamma + delta, 2 % substitutions, R1 mode: both chains switch to the `original` tag set, each in its own copy of
    the arguments."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dec, "BATCH_READS", 300)
    tg, td = synth.config5_tagsets()
    for ts in (tg, td):
        ts.write(str(tmp_path / "tags"))
    chu.write_synth_pair(tmp_path, (tg, td), 500, seed=51, sub_rate=0.02, n_long=3, r1_mode=True)
    got = chu.compare_with_single_runs(tmp_path, "g,d", ["-in", "SYN_1.fq", "-br", "R1", "-tfdir", "tags", "-sp", "mouse",
                                                          "-or", "both", "-dc"])
    assert {"dcr_SYN_1_gamma.n12", "dcr_SYN_1_delta.n12"} <= set(got)
    assert dec.chain_args["g"]["tags"] == dec.chain_args["d"]["tags"] == "original"


def test_tags_rewrite_stays_with_its_chain(tmp_path, monkeypatch, oracle_device):
    """Human beta (extended) with mouse-free gamma: only gamma's copy switches to `original`."""
    monkeypatch.chdir(tmp_path)
    tb = synth.config3_tagsets()[1]
    tg = synth.make_tagset("human", "original", "g", n_v=12, n_j=4, seed=20260106, n_shared_groups=2)
    for ts in (tb, tg):
        ts.write(str(tmp_path / "tags"))
    chu.write_synth_pair(tmp_path, (tb, tg), 200, seed=61)
    args = dio.create_args_dict(infile="SYN_1.fq", chain="b,g", bc_read="R2", dontgzip=True, dontcount=True,
                                tagfastadir="tags", outpath="", command="decombine")
    dec.decombinator_chains(args)
    assert args["tags"] == "extended"
    assert dec.chain_args["b"]["tags"] == "extended" and dec.chain_args["g"]["tags"] == "original"
    logs = {p.name: p.read_text() for p in (tmp_path / "Logs").glob("*.csv")}
    assert any("_beta_" in k and "\ntags,extended\n" in v for k, v in logs.items())
    assert any("_gamma_" in k and "\ntags,original\n" in v for k, v in logs.items())


def test_empty_input_writes_every_chains_log(tmp_path, monkeypatch, oracle_device):
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    (tmp_path / "empty_1.fq").write_text("")
    args = dio.create_args_dict(infile="empty_1.fq", chain="a,b", bc_read="R2", tagfastadir="tags", outpath="")
    with pytest.raises(ValueError, match="fewer than four lines"):
        dec.decombinator_chains(args)
    names = sorted(p.name for p in (tmp_path / "Logs").glob("*.csv"))
    assert len(names) == 2 and "_alpha_empty_1_" in names[0] and "_beta_empty_1_" in names[1]


# ---- refusals and parsing ------------------------------------------------------------------------------------------

def test_chain_list_parsing():
    assert dec.chain_list("a,b") == ["a", "b"] and dec.chain_list("b") is None and dec.chain_list(None) is None
    assert dec.resolve_chain_list(["alpha", "TRB"]) == ["a", "b"]
    assert dec.resolve_chain_list(dec.chain_list("g, tcrd,A,beta")) == ["g", "d", "a", "b"]
    with pytest.raises(ValueError, match="named twice"):
        dec.resolve_chain_list(["b", "beta"])
    with pytest.raises(ValueError, match="not a chain"):
        dec.resolve_chain_list(["a", "x"])
    a = dio.cli_args(["decombine", "-in", "x_1.fq", "-br", "R2", "-c", "a,b"])
    assert a["chain"] == "a,b"
    p = dio.cli_args(["pipeline", "-in", "x_1.fq", "-br", "R2", "-c", "alpha,beta", "--cluster"])
    assert p["chain"] == "alpha,beta" and p["cluster"] is True
    assert dio.create_args_dict(infile="x_1.fq", chain="a,b", bc_read="R2")["chain"] == "a,b"


def test_refusals_before_anything_is_read(tmp_path, monkeypatch, oracle_device):
    monkeypatch.chdir(tmp_path)
    chu.tiny_workdir(tmp_path)
    opened = []
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: opened.append(a) or pytest.fail("a reader was opened"))
    base = dio.create_args_dict(infile="TINY_1.fq", chain="b,beta", bc_read="R2", tagfastadir="tags", outpath="")
    with pytest.raises(ValueError, match="named twice"):
        dec.decombinator_chains(dict(base))
    with pytest.raises(ValueError, match="not a chain"):
        dec.decombinator_chains(dict(base, chain="a,b,x"))
    for argv in (["decombine", "-in", "TINY_1.fq", "-br", "R2", "-c", "b,beta", "-tfdir", "tags"],
                 ["pipeline", "-in", "TINY_1.fq", "-br", "R2", "-c", "a,a", "-tfdir", "tags"],
                 ["collapse", "-in", "dcr_TINY_1_alpha.n12", "-c", "a,b", "--cluster"],
                 ["translate", "-in", "dcr_TINY_1_alpha.freq", "-c", "a,b"]):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
    with pytest.raises(ValueError, match="sharded"):
        sharded.decombinator_sharded(dict(base, chain="a,b"), comm=None)
    # decombinator() keeps its one-chain contract: a list is the reference's chain error there
    with pytest.raises(SystemExit):
        dec.decombinator(dict(base, chain="a,b"))
    assert opened == []


def test_cli_refusal_messages(capsys):
    for argv, msg in ((["collapse", "-in", "x.n12", "-c", "a,b"], "one per-chain file"),
                      (["decombine", "-in", "x_1.fq", "-br", "R2", "-c", "b,beta"], "named twice")):
        with pytest.raises(SystemExit):
            pipeline.main(argv)
        assert msg in capsys.readouterr().err


# ---- the C entry's argument errors (codes, never an abort; no GPU needed) --------------------------------------------

def test_decombine_chains_argument_errors():
    L = nat.lib()
    fx = json.load(open(os.path.join(chu.HERE, "golden", "tiny_alpha.json")))["tagset"]
    from tests import parity_util as pu
    ta, tb = pu.native_tables(fx), pu.native_tables(fx)
    batch = nat.pack_reads(["ACGT" * 30])
    b = batch.as_c()
    cfg = nat.make_cfg()
    rec = [nat.np.zeros(1, dtype=nat.RECORD_DTYPE) for _ in range(5)]
    cnt = [nat.np.zeros(nat.N_COUNTERS, dtype=nat.np.uint64) for _ in range(5)]

    def call(handles, n, recs=rec, cnts=cnt, batch_c=C.byref(b), cfg_c=C.byref(cfg)):
        hs = (C.c_void_p * 5)(*handles) if handles is not None else None
        rp = (C.c_void_p * 5)(*[r.ctypes.data for r in recs]) if recs is not None else None
        cp = (C.c_void_p * 5)(*[c.ctypes.data for c in cnts]) if cnts is not None else None
        return L.dcrx_decombine_chains(hs, n, cfg_c, batch_c, rp, cp)

    h = [ta.handle, tb.handle]
    assert call(h, 0) == -1 and b"n_chains" in L.dcrx_last_error()
    assert call(h + [None] * 3, 5) == -1 and b"n_chains" in L.dcrx_last_error()
    assert call(None, 2) == -1
    assert call(h, 2, recs=None) == -1
    assert call(h, 2, cnts=None) == -1
    assert call(h, 2, cfg_c=None) == -1
    assert call([ta.handle, None], 2) == -1
    assert call([ta.handle, ta.handle], 2) == -1 and b"same tables handle" in L.dcrx_last_error()
    with pytest.raises(nat.DcrxError) as e:
        nat.decombine_chains([ta, ta], batch)
    assert e.value.code == -1
    with pytest.raises(nat.DcrxError) as e:
        nat.decombine_chains([ta, tb] * 3, batch)
    assert e.value.code == -1
    b2 = nat.pack_reads(["ACGT" * 30]).as_c()
    b2.stride = 12
    assert L.dcrx_decombine_chains((C.c_void_p * 2)(*h), 2, C.byref(cfg), C.byref(b2),
                                   (C.c_void_p * 2)(rec[0].ctypes.data, rec[1].ctypes.data),
                                   (C.c_void_p * 2)(cnt[0].ctypes.data, cnt[1].ctypes.data)) == -1
