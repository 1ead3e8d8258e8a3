"""The clonotype step (`translate --clonotypes`, `pipeline --clonotypes`) on the CPU: the per-entry code the kernels run
(dcrx_clono_core.h built by g++, tests/host_clono) against dcrx_cdr3_batch field by field, the contract's brute force
(cu.expected_clonotypes) on hand-made tables, libdcrx's host formatter, and the stage — flag, refusals, file — with the brute
force standing in for _native.clonotypes (the one function that needs the GPU)."""
import collections
import gzip
import json
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import io as dio
from decombinator_amd import pipeline, synth, translate
from tests import clonotype_util as cu
from tests import collapse_cluster_util as ccu
from tests import golden_util as gu
from tests import nbc_count_util as nu
from tests import parity_util as pu


# ---- the per-entry code against dcrx_cdr3_batch ----

def test_host_build_equals_cdr3_batch_on_every_golden_case():
    G = cu.golden_genes()
    n = 0
    for tab, index_error, cases in cu.golden_case_tables():
        rows, arena = cu.host_calls(G, tab)
        seen = cu.assert_rows_equal_batch(G, tab, rows, arena)
        assert [bool(r["status"] == nat.CDR3_INDEX_ERROR) for r in rows] == index_error
        # ... and against the fixture itself: the reference's junctions
        at = 0
        for r, c in zip(rows, cases):
            if c["expect"] != "IndexError" and c["expect"]["productive"] == "T":
                want = (c["expect"]["junction_aa"] + c["expect"]["junction"]).encode()
                assert arena[at:at + len(want)] == want and r["flags"] & 1
                at += len(want)
        n += sum(seen.values())
    assert n == 1308


def test_host_build_equals_cdr3_batch_on_the_coding_dcrs():
    G, tab, fx = cu.coding_table()
    rows, arena = cu.host_calls(G, tab)
    cu.assert_rows_equal_batch(G, tab, rows, arena)
    assert len(rows) == 513 and int((rows["flags"] & 1).sum()) == 371 == sum(e["productive"] == "T" for e in fx["expect"])


def test_host_build_on_ambiguity_codes_gaps_and_motifs():
    seen = collections.Counter()
    for G, tab in [cu.ambiguity_case(), cu.ambiguous_insert_case(), cu.gap_case()] + [(g, t) for _, g, t in cu.motif_cases()]:
        rows, arena = cu.host_calls(G, tab)
        seen.update(cu.assert_rows_equal_batch(G, tab, rows, arena))
    assert all(seen[s] > 20 for s in (nat.CDR3_OK, nat.CDR3_INDEX_ERROR, nat.CDR3_BAD_CODON, nat.CDR3_MOTIF_LEFT))
    G = cu.coding_genes(3)
    tab = cu.random_table(G, 3000, seed=2, max_del=20, max_ins=12)
    rows, arena = cu.host_calls(G, tab)
    assert cu.assert_rows_equal_batch(G, tab, rows, arena)[nat.CDR3_OK] == len(rows) and (rows["flags"] & 1).sum() > 300


def test_keys_compare_in_full_and_equal_keys_hash_equal():
    """Two alleles of one gene share a call group: the same junction_aa under them is ONE key (equal hashes, equal in full);
    under another gene, or with another residue, it is not — whatever the hashes say."""
    G = cu.coding_genes(3)
    cut = lambda v: len(G.v_regions[v]) - 273           # the V region up to and including the conserved C's codon
    back = lambda j: "AC"[:(-(len(G.j_regions[j]) - 49)) % 3]
    rows = [(0, 2, cut(0), 0, "GCAGGT" + back(2), 1), (1, 2, cut(1), 0, "GCCGGA" + back(2), 1), (2, 2, cut(2), 0, "GCAGGT" + back(2), 1),
            (0, 2, cut(0), 0, "GCAGAT" + back(2), 1)]
    tab = cu.table(rows)
    r, arena = cu.host_calls(G, tab)
    assert (r["flags"] & 1).all()
    f = nat.clono_row_fields(r)
    ja = [arena[int(x["arena_off"]):int(x["arena_off"]) + int(y["junction_aa_len"])] for x, y in zip(r, f)]
    assert ja[0] == ja[1] == ja[2] != ja[3] and ja[0].startswith(b"CAG")
    assert r["hash"][0] == r["hash"][1] and len(set(r["hash"].tolist())) == 3
    genes = translate._native_genes(G)
    vg, jg = nat.call_groups(G.v_names), nat.call_groups(G.j_names)
    assert vg[0] == vg[1] != vg[2] and jg[0] == jg[1] != jg[2]
    import ctypes as C
    eq = lambda a, b: cu.host_lib().clono_host_key_equal(C.byref(genes.c), vg.ctypes.data, jg.ctypes.data, rows[a][0], rows[a][1], len(ja[a]),
                                                         ja[a], rows[b][0], rows[b][1], len(ja[b]), ja[b])
    assert eq(0, 1) == 1 and eq(0, 2) == 0 and eq(0, 3) == 0 and eq(3, 3) == 1


# ---- constructed junction geometry (cu.geometry_case): where each residue and each verdict is read from ----

def test_host_build_on_the_full_geometry_product():
    """13 V x 12 J small genes (cu.GEOMETRY_V, cu.GEOMETRY_J), every vdel in -2 .. len(V) + 2, every jdel in -2 .. len(J) + 2,
    28 inserts, and the gene indices -1, -n, -n - 1, n: 1 346 592 rows, of which dcrx_cdr3_batch calls 823 645 OK, 149 221
    INDEX_ERROR and 373 726 BAD_CODON.  Every shared field, arena_off and every junction byte of the host build, exactly."""
    G, tab = cu.geometry_case()
    rows, arena = cu.host_calls(G, tab)
    seen = cu.assert_rows_equal_batch(G, tab, rows, arena)
    assert len(rows) == 1_346_592 and seen == {nat.CDR3_OK: 823_645, nat.CDR3_INDEX_ERROR: 149_221, nat.CDR3_BAD_CODON: 373_726, nat.CDR3_MOTIF_LEFT: 0}


def test_thinned_geometry_list_keeps_its_premises_and_the_reference_is_anchored():
    """One row in cu.GEOMETRY_STRIDE of the product (122 483 rows; the list the GPU test runs): the premises as
    cu.geometry_premises counts them on dcrx_cdr3_batch's rows and the plain Python model — 74 951 OK, 13 527 INDEX_ERROR,
    34 005 BAD_CODON; all 16 flag combinations; 1 749 productive; the rarest edge class (the first invalid V codon at index
    nv, none read) 869 rows.  dcrx_cdr3_batch itself against translate.cdr3_batch's records and against cu.plain_call, which
    joins and translates in Python, on every 17th row (7 205)."""
    G, tab = cu.geometry_case(thin=True)
    n = cu.geometry_premises(G, tab)
    assert n["status"][nat.CDR3_MOTIF_LEFT] == 0 and min(n["classes"].values()) == n["classes"]["v_bad_at_nv_no_bad"] == 869
    assert cu.sample_agrees_with_python_calls(G, tab, 17) >= 3000
    rows, arena = cu.host_calls(G, tab)
    cu.assert_rows_equal_batch(G, tab, rows, arena)


@pytest.mark.parametrize("case", ["geometry", "coding"])
def test_respelt_twins_are_one_answer_on_the_host_build(case):
    """One sequence spelt as several DCRs (cu.respelt_twins: bases moved from the V piece or the J piece into the insert): the
    residues move between the V table, direct_aa and the (J, phase) table, k0 and the phase change, the calls may not.
    geometry: 400 sets, 5 080 rows, 150 sets productive.  coding: 300 sets of 22 spellings, all productive, each with the
    conserved C's codon read from the V table, straddling the V / insert edge, and from the insert."""
    G, sets = cu.geometry_twins() if case == "geometry" else cu.coding_twins()
    tab, where = cu.twin_table(sets)
    rows, arena = cu.host_calls(G, tab)
    cu.assert_rows_equal_batch(G, tab, rows, arena)
    productive = cu.assert_twins_agree(rows, arena, where)
    assert (len(sets), productive) == ((400, 150) if case == "geometry" else (300, 300))
    assert cu.assert_twin_sets_share_a_clonotype(cu.expected_clonotypes(tab, G), where) == productive


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_mixed_block_tables_hold_their_premises(n):
    """cu.mixed_block_table, the tables of the GPU suite's mixed-geometry block-edge test, on the reference side and the host
    build: 40 twin sets that are 40 clonotypes, non-members of both kinds (a stop in frame or out of frame; a bad codon)."""
    G, tab, where = cu.mixed_block_table(n)
    rows, arena = cu.host_calls(G, tab)
    seen = cu.assert_rows_equal_batch(G, tab, rows, arena)
    want = cu.expected_clonotypes(tab, G)
    assert cu.assert_twins_agree(rows, arena, where) == cu.assert_twin_sets_share_a_clonotype(want, where) == want[1]["clonotypes_out"] == 40
    assert seen[nat.CDR3_BAD_CODON] == want[1]["untranslatable"] > 20 and want[1]["nonproductive"] > 20
    assert len(set(tab["count"].tolist())) == n


def test_pyslice_is_pythons_slice():
    """make_entry's J slice with a deletion longer than the gene takes nothing whichever way `start > n` is clamped (no base
    and no table entry is read behind it), so no table can tell; the function itself can."""
    import ctypes as C
    lo, hi = C.c_int64(), C.c_int64()
    for n in range(0, 6):
        for start in range(-8, 9):
            for stop in range(-8, 9):
                cu.host_lib().clono_host_pyslice(n, start, stop, C.byref(lo), C.byref(hi))
                a, b, _ = slice(start, stop).indices(n)
                assert (lo.value, hi.value) == (a, max(a, b)), (n, start, stop)


# ---- the contract's brute force on hand-made tables ----

def _hand_rows(G):
    cut = lambda v: len(G.v_regions[v]) - 273
    back = lambda j: "AC"[:(-(len(G.j_regions[j]) - 49)) % 3]
    return [
        (0, 2, cut(0), 0, "GCAGGT" + back(2), 9),       # 0  CAG...: the representative of row A (count 9)
        (1, 2, cut(1), 0, "GCCGGA" + back(2), 9),       # 1  the same CDR3, synonymous codons, the other allele: joins A; a tie in count
        (2, 2, cut(2), 0, "GCAGGT" + back(2), 9),       # 2  the same CDR3 under another V gene: row B
        (0, 2, cut(0), 0, "GCAGAT" + back(2), 7),       # 3  another CDR3: row C
        (0, 2, cut(0), 0, "TAAGGT" + back(2), 50),      # 4  a stop: non-productive
        (0, 2, cut(0), 0, "GCTGGG" + back(2), 2),       # 5  joins A
        (3, 3, 0, 0, "ACJ", 4),                         # 6  no nucleotide code: untranslatable
        (0, 2, cut(0), 0, "GCAGAA" + back(2), 7),       # 7  the same count as row C, a later rank: row D behind it
    ]


def test_hand_made_table():
    G = cu.coding_genes(3)
    tabl, stats, of = cu.expected_clonotypes(cu.table(_hand_rows(G)), G)
    assert tabl["rep"].tolist() == [0, 2, 3, 7]
    assert tabl["duplicate_count"].tolist() == [20, 9, 7, 7] and tabl["n_dcrs"].tolist() == [3, 1, 1, 1]
    assert tabl["top_dcr_count"].tolist() == [9, 9, 7, 7]
    assert of.tolist() == [0, 0, 1, 2, nat.NOT_A_MEMBER, 0, nat.NOT_A_MEMBER, 3]
    assert tabl["junction_aa"][0] == tabl["junction_aa"][1] and tabl["v_call"][:2] == ["TRBV1", "TRBV2"]
    assert tabl["junction"][0].startswith("TGTGCAGGT")
    assert stats == dict(entries_in=8, reads_in=97, productive=6, productive_reads=43, nonproductive=1, nonproductive_reads=50,
                         untranslatable=1, untranslatable_reads=4, clonotypes_out=4, convergent=1, largest_n_dcrs=3)


def test_tables_without_a_clonotype():
    G = cu.coding_genes(3)
    for rows in ([], [_hand_rows(G)[4]], [_hand_rows(G)[6]]):
        tabl, stats, of = cu.expected_clonotypes(cu.table(rows), G)
        assert len(tabl["rep"]) == 0 and stats["clonotypes_out"] == 0 and stats["entries_in"] == len(rows)
        assert (of == nat.NOT_A_MEMBER).all()


# ---- the host pieces of the native side ----

def test_format_clonotypes_and_the_gene_set_need_no_device():
    G = cu.coding_genes(3)
    tab = cu.table(_hand_rows(G))
    native = cu.brute_force_native(G)
    genes = translate._clono_genes(G)
    table, stats, of = native(genes, tab)
    text = nat.format_clonotypes(genes, table, tab).decode()
    assert text == cu.file_text(cu.expected_clonotypes(tab, G)[0], tab)
    assert text.splitlines()[0].split("\t") == nat.CLONOTYPE_COLUMNS
    assert text.splitlines()[1].split("\t")[6] == ", ".join(str(x) for x in _hand_rows(G)[0][:5])       # no blank in front
    empty = cu.table([])
    assert nat.format_clonotypes(genes, native(genes, empty)[0], empty).decode() == "\t".join(nat.CLONOTYPE_COLUMNS) + "\n"
    # the empty table needs no device either
    got = nat.clonotypes(genes, empty)
    assert len(got[0]["rep"]) == 0 and got[1] == dict.fromkeys(nat.CLONOTYPE_STATS, 0) and len(got[2]) == 0
    assert nat.clono_work_bytes(1 << 31, 0) == 0
    with pytest.raises(nat.DcrxError, match="0 .. 64"):
        genes.set_hash_bits(65)
    with pytest.raises(ValueError, match="one name per gene"):
        nat.ClonoGenes(translate._native_genes(G), G.v_names[:-1], G.j_names)
    assert nat.CLONO_ROW_DTYPE.itemsize == 32 and nat.ABI_VERSION == nat.lib().dcrx_abi_version()


# ---- the stage, with the brute force as _native.clonotypes ----

@pytest.fixture()
def coding(tmp_path, monkeypatch):
    """The coding fixture as files in a working directory, the oracle as the device, the brute force as _native.clonotypes."""
    monkeypatch.chdir(tmp_path)
    fx = json.load(open(cu.CODING_FX))
    ts = fx["tagset"]
    t = synth.TagSet(species=ts["species"], tags=ts["tags"], chain=ts["chain"], v_tags=ts["v_tags"], v_jumps=ts["v_jumps"],
                     v_names=ts["v_names"], v_regions=ts["v_regions"], j_tags=ts["j_tags"], j_jumps=ts["j_jumps"],
                     j_names=ts["j_names"], j_regions=ts["j_regions"])
    cu.write_gene_files(tmp_path / "tags", t, fx["genes"])
    (tmp_path / "COD_1.fq").write_text(fx["fastq_r1"])
    (tmp_path / "COD_2.fq").write_text(fx["fastq_r2"])
    G = translate.GeneInfo(**fx["genes"])
    calls = []

    def clonotypes(genes, counted):
        calls.append(len(counted["v"]))
        return cu.brute_force_native(G)(genes, counted)
    monkeypatch.setattr(nat, "clonotypes", clonotypes)
    ot = gu.oracle_tables(ts)
    monkeypatch.setattr(nat, "decombine", lambda tables, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0:
                        pu.oracle_records(ot, nat.unpack_reads(batch), orientation, allow_ns, lenthreshold))
    monkeypatch.setattr(nat, "umi_neighbours", ccu.brute_neighbours)
    common = ["-tfdir", "tags", "-tg", ts["tags"], "-sp", ts["species"], "-c", ts["chain"]]
    return fx, G, calls, common


def _want_file(G, rows):
    """The file's text for rows (v, j, vdel, jdel, insert, count) in rank order."""
    tab = cu.table(rows)
    return cu.file_text(cu.expected_clonotypes(tab, G)[0], tab)


def _counted_rows(fx):
    reads = fx["fastq_r1"].splitlines()[1::4]
    keys, _ = nu.read_dcrs(gu.oracle_tables(fx["tagset"]), reads)
    out = []
    for k, n in collections.Counter(k for k in keys if k is not None).most_common():
        f = k.split(", ")
        out.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), f[4], n))
    return out


def test_pipeline_count_dcrs_then_translate_over_the_nbc(coding, monkeypatch, tmp_path):
    fx, G, calls, common = coding
    nu.OracleCountDevice(monkeypatch)
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-dc", "-s", "-dz"] + common)
    rows = _counted_rows(fx)
    want = _want_file(G, rows)
    name = tmp_path / "dcr_COD_1_beta.clonotypes.tsv"
    assert name.read_text() == want and len(want.splitlines()) > 300
    assert oct(os.stat(name).st_mode & 0o777) == "0o666"
    assert calls == [len(rows)] and translate.clonotype_stats["entries_in"] == len(rows)
    assert translate.chain_clonotype_stats["b"] == translate.clonotype_stats
    assert sum(int(ln.split("\t")[3]) for ln in want.splitlines()[1:]) == translate.clonotype_stats["productive_reads"]
    # translate over the `.nbc` that run wrote: the same table, named after the input file, gzipped by default
    pipeline.main(["translate", "-in", "dcr_COD_1_beta.nbc", "-nbc", "--count-dcrs", "--clonotypes"] + common)
    assert gzip.open(tmp_path / "dcr_COD_1_beta.clonotypes.tsv.gz", "rt").read() == want
    assert (tmp_path / "dcr_COD_1_beta.tsv.gz").exists() and calls == [len(rows)] * 2


def test_pipeline_cluster_then_translate_over_the_freq(coding, tmp_path):
    fx, G, calls, common = coding
    for name, text in zip(("BC_1.fq", "BC_2.fq"), cu.barcoded_pair(fx)):
        (tmp_path / name).write_text(text)
    pipeline.main(["pipeline", "-in", "BC_1.fq", "-br", "R2", "--cluster", "--clonotypes", "-dc", "-s", "-dz", "-ol", "M13"] + common)
    freq = [ln.split(", ") for ln in (tmp_path / "dcr_BC_1_beta.freq").read_text().splitlines()]
    assert len(freq) > 400 and max(int(f[5]) for f in freq) >= 3
    want = _want_file(G, [(int(f[0]), int(f[1]), int(f[2]), int(f[3]), f[4], int(f[5])) for f in freq])
    assert (tmp_path / "dcr_BC_1_beta.clonotypes.tsv").read_text() == want
    os.mkdir(tmp_path / "out")
    pipeline.main(["translate", "-in", "dcr_BC_1_beta.freq", "--clonotypes", "-dz", "-op", "out" + os.sep] + common)
    assert (tmp_path / "out" / "dcr_BC_1_beta.clonotypes.tsv").read_text() == want
    assert calls == [len(freq)] * 2


def test_without_the_flag_nothing_is_written_or_called(coding, monkeypatch, tmp_path):
    fx, G, calls, common = coding
    nu.OracleCountDevice(monkeypatch)
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "-dc", "-s", "-dz"] + common)
    pipeline.main(["translate", "-in", "dcr_COD_1_beta.nbc", "-nbc", "--count-dcrs", "-dz"] + common)
    assert calls == []
    assert not [x for x in os.listdir(tmp_path) if "clonotypes" in x]
    assert dio.create_args_dict(infile="x", chain="b", bc_read="R2")["clonotypes"] is False
    assert dio.cli_args(["translate", "-in", "x.freq"])["clonotypes"] is False


def test_dontsave_keeps_the_statistics_and_writes_nothing(coding, monkeypatch, tmp_path):
    fx, G, calls, common = coding
    nu.OracleCountDevice(monkeypatch)
    pipeline.main(["pipeline", "-in", "COD_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-dc", "-s", "-ds"] + common)
    assert len(calls) == 1 and translate.clonotype_stats["productive"] == 371
    assert not [x for x in os.listdir(tmp_path) if "clonotypes" in x]


def test_two_chains_write_their_own_files(tmp_path, monkeypatch):
    """`pipeline -c a,b -nbc --count-dcrs --clonotypes`: each chain's file equals its single-chain run's.  The synthetic pair of
    tag sets carries no translate gene tables (and its random regions are full of stops): the gene import is fed a seeded
    coding gene set per chain with as many genes as the chain's tag set has."""
    monkeypatch.chdir(tmp_path)
    nu.OracleCountDevice(monkeypatch)
    ta, tb = synth.config3_tagsets()
    sets = {"a": ta, "b": tb}

    infos = {c: cu.coding_genes(40 + k, len(ts.v_regions), len(ts.j_regions)) for k, (c, ts) in enumerate(sets.items())}
    monkeypatch.setattr(translate, "import_gene_information", lambda inputargs: infos[inputargs["chain"]])
    monkeypatch.setattr(nat, "clonotypes", lambda genes, counted: cu.brute_force_native(translate._genes)(genes, counted))
    reads = nu.clonal_reads(ta, 300, seed=31) + nu.clonal_reads(tb, 300, seed=32)
    ta.write(str(tmp_path / "tags"))
    tb.write(str(tmp_path / "tags"))
    nu.write_fastq(tmp_path / "NBC_1.fq", reads)
    base = ["pipeline", "-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "--clonotypes", "-tfdir", "tags", "-tg", ta.tags, "-sp", ta.species,
            "-dc", "-s", "-dz"]
    pipeline.main(base + ["-c", "a,b"])
    both = {c: (tmp_path / f"dcr_NBC_1_{n}.clonotypes.tsv").read_text() for c, n in (("a", "alpha"), ("b", "beta"))}
    stats = {c: dict(translate.chain_clonotype_stats[c]) for c in "ab"}
    for c, n in (("a", "alpha"), ("b", "beta")):
        os.remove(tmp_path / f"dcr_NBC_1_{n}.clonotypes.tsv")
        pipeline.main(base + ["-c", c])
        assert (tmp_path / f"dcr_NBC_1_{n}.clonotypes.tsv").read_text() == both[c]
        assert translate.clonotype_stats == stats[c] and stats[c]["entries_in"] > 20 and stats[c]["clonotypes_out"] > 3
    assert both["a"] != both["b"]


def test_refusals_before_anything_is_read(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(nat, "FastqReader", lambda *a, **k: pytest.fail("a reader was opened"))
    monkeypatch.setattr(translate, "import_gene_information", lambda *a, **k: pytest.fail("gene files were read"))
    monkeypatch.setattr(nat, "clonotypes", lambda *a, **k: pytest.fail("the device was called"))
    import builtins
    real_open = builtins.open
    monkeypatch.setattr(gzip, "open", lambda *a, **k: pytest.fail("a file was opened"))
    fq = ["-in", "X_1.fq", "-br", "R2", "-c", "b", "-tfdir", "tags", "--clonotypes"]
    for argv, msg in ((["decombine"] + fq, "does not translate"),
                      (["decombine"] + fq + ["-nbc", "--count-dcrs"], "does not translate"),
                      (["collapse", "-in", "dcr_X_1_beta.n12", "-c", "b", "--clonotypes", "--cluster"], "does not translate"),
                      (["pipeline"] + fq, "--cluster"),
                      (["pipeline"] + fq + ["-nbc"], "--count-dcrs"),
                      (["translate", "-in", "dcr_X_1_beta.nbc.gz", "-c", "b", "-nbc", "--clonotypes"], "every row would count 1")):
        with pytest.raises(SystemExit) as e:
            pipeline.main(argv)
        assert e.value.code == 2, argv
    assert builtins.open is real_open and os.listdir(tmp_path) == []
    args = dio.create_args_dict(infile="X_1.fq", chain="b", bc_read="R2", tagfastadir="tags", outpath="", command="pipeline", clonotypes=True)
    with pytest.raises(ValueError, match="--cluster"):
        pipeline.run(args)
    assert "every row would count 1" in pipeline.clonotype_refusal(dict(args, command="translate", nobarcoding=True))
    assert pipeline.clonotype_refusal(dict(args, command="translate")) is None
    assert pipeline.clonotype_refusal(dict(args, cluster=True)) is None and pipeline.clonotype_refusal(dict(args, clonotypes=False)) is None


def test_an_unserved_motif_is_a_clear_error(monkeypatch):
    G = cu.coding_genes(3)

    def refuse(genes, counted):
        raise nat.DcrxError(-2, "dcrx_clonotypes: entry 0 uses J gene 4, whose motif '(F|W)G.G' needs a regular-expression engine")
    monkeypatch.setattr(nat, "clonotypes", refuse)
    with pytest.raises(translate.UnsupportedMotif, match=r"\(F\|W\)G\.G"):
        translate.clonotypes({}, cu.table(_hand_rows(G)), G)
