"""What the clonotype tests share (`translate --clonotypes`, include/dcrx.h "clonotypes"): the contract as a brute force in
Python on top of translate.cdr3_batch, table and gene-set generators, the host build of the per-entry code
(tests/host_clono), and the comparison of its rows with dcrx_cdr3_batch's."""
import ctypes as C
import json
import os
import random

import numpy as np

from decombinator_amd import _native as nat
from decombinator_amd import translate

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "translate_cdr3.json")
CODING_FX = os.path.join(HERE, "golden", "translate_stage_coding.json")
HOST_LIB = os.path.join(HERE, "host_clono", "build", "libclono_host.so")


def golden_genes(**over) -> translate.GeneInfo:
    g = dict(json.load(open(GOLDEN))["genes"])
    g.update(over)
    return translate.GeneInfo(**g)


def gene_info(v_regions, j_regions, v_pos, v_res, j_pos, j_motif, v_names=None, j_names=None) -> translate.GeneInfo:
    nv, nj = len(v_regions), len(j_regions)
    return translate.GeneInfo(v_regions=list(v_regions), j_regions=list(j_regions),
                              v_names=list(v_names) if v_names else [f"TRBV{k + 1}*01" for k in range(nv)],
                              j_names=list(j_names) if j_names else [f"TRBJ{k + 1}*01" for k in range(nj)],
                              v_translate_position=list(v_pos), v_translate_residue=list(v_res), j_translate_position=list(j_pos),
                              j_translate_residue=list(j_motif), v_functionality=["F"] * nv, j_functionality=["F"] * nj,
                              v_cdr1=[""] * nv, v_cdr2=[""] * nv)


# ---- tables ----

def table(rows) -> dict:
    """The counted table (what DcrCounts.read() gives, as far as the clonotype step reads it) of rows (v, j, vdel, jdel,
    insert, count), in the order given: row k has rank k."""
    ib = [str(r[4]).encode("latin-1") for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in ib])
    return {"v": np.array([r[0] for r in rows], dtype=np.int32), "j": np.array([r[1] for r in rows], dtype=np.int32),
            "vdel": np.array([r[2] for r in rows], dtype=np.int32), "jdel": np.array([r[3] for r in rows], dtype=np.int32),
            "count": np.array([r[5] for r in rows], dtype=np.uint64), "ins_off": off, "ins_text": b"".join(ib)}


def table_rows(tab: dict) -> list:
    text, off = tab["ins_text"], tab["ins_off"]
    return [(int(tab["v"][k]), int(tab["j"][k]), int(tab["vdel"][k]), int(tab["jdel"][k]),
             text[int(off[k]):int(off[k + 1])].decode("latin-1"), int(tab["count"][k])) for k in range(len(tab["v"]))]


def random_table(G: translate.GeneInfo, n: int, seed: int, max_del: int = 9, max_ins: int = 7) -> dict:
    """n draws of a random DCR over G's genes, the distinct ones kept, with Zipf-like counts, in count-descending order (a
    counted table's rank order).  Inserts are drawn so that about a third of the sequences are in frame."""
    rnd = random.Random(seed)
    seen = {}
    for _ in range(n):
        d = (rnd.randrange(len(G.v_regions)), rnd.randrange(len(G.j_regions)), rnd.randrange(max_del + 1), rnd.randrange(max_del + 1),
             "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(max_ins + 1))))
        if d not in seen:
            seen[d] = max(1, int(1000 / (1 + rnd.paretovariate(1.2) * len(seen) / 50)))
    rows = [d + (c,) for d, c in seen.items()]
    rows.sort(key=lambda r: -r[5])       # (stable: ties stay in draw order)
    return table(rows)


_SENSE = [a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG" if a + b + c not in ("TAA", "TAG", "TGA")]


def coding_genes(seed: int, n_v: int = 8, n_j: int = 5, v_codons: int = 95, j_codons: int = 16) -> translate.GeneInfo:
    """A seeded gene set that codes: stop-free V and J regions drawn from sense codons, the conserved C planted at the V
    position (a few codons before the V region's end) and an FG.G motif in every J; the first two V genes and the first two J
    genes are two alleles of one gene (*01, *02: one call), with different bases."""
    rnd = random.Random(seed)
    vr, vp, vn = [], [], []
    for k in range(n_v):
        codons = [rnd.choice(_SENSE) for _ in range(v_codons)]
        pos = v_codons - 4
        codons[pos - 1] = "TGT"
        vr.append("".join(codons) + rnd.choice(["", "A", "GC"]))
        vp.append(pos)
        vn.append(f"TRBV{max(k, 1)}*0{2 if k == 1 else 1}")
    jr, jp, jn = [], [], []
    for k in range(n_j):
        lead = rnd.randrange(3)
        codons = [rnd.choice(_SENSE) for _ in range(j_codons)]
        codons[4:8] = ["TTT", "GGA", rnd.choice(_SENSE), "GGG"]
        # (len - 1) % 3 == 0 is the reference's frame test: one base behind the last whole codon
        jr.append("".join(rnd.choice("ACGT") for _ in range(lead)) + "".join(codons) + "C")       # (49 bases behind the lead)
        jp.append(-(j_codons - 4))
        jn.append(f"TRBJ{max(k, 1)}*0{2 if k == 1 else 1}")
    return gene_info(vr, jr, vp, ["C"] * n_v, jp, ["FG.G"] * n_j, vn, jn)


def coding_insert(G: translate.GeneInfo, v: int, j: int, codons: str) -> str:
    """An insert for whole V and J regions of coding_genes() that keeps `codons` in frame: bases that fill the V region's last
    codon in front, bases that put the J region's codons in frame behind (neither can make a stop)."""
    front = "ACG"[:(-len(G.v_regions[v])) % 3]
    back = "AC"[:(-(len(G.j_regions[j]) - 49)) % 3]
    return front + codons + back


def write_gene_files(tags_dir, tagset, genes: dict) -> None:
    """A tag set's files (synth.TagSet.write) with the `.translate` and `.cdrs` files import_gene_information reads."""
    tagset.write(str(tags_dir))
    stem = f"{tagset.species}_{tagset.tags}_TR{tagset.chain.upper()}"
    for gene, names, pos, res, fun in (("V", genes["v_names"], genes["v_translate_position"], genes["v_translate_residue"], genes["v_functionality"]),
                                       ("J", genes["j_names"], genes["j_translate_position"], genes["j_translate_residue"], genes["j_functionality"])):
        with open(os.path.join(str(tags_dir), f"{stem}{gene}.translate"), "w") as fh:
            for n, p_, r, f in zip(names, pos, res, fun):
                fh.write(f"{n},{p_},{r},{f}\n")
    with open(os.path.join(str(tags_dir), f"{stem}V.cdrs"), "w") as fh:
        for n, a, b in zip(genes["v_names"], genes["v_cdr1"], genes["v_cdr2"]):
            fh.write(f"{n} {a} {b}\n")


def barcoded_pair(fx: dict, seed: int = 4):
    """(R1 text, R2 text) of a barcoded run over the coding fixture's own R1 reads.  The fixture's R2 reads carry no M13
    spacers (collapse would drop every read), so each R1 read is written one to three times, every copy with a molecule of its
    own: an R2 read that starts with the M13 oligo's spacers around two random six-base UMI halves."""
    rnd = random.Random(seed)
    s1, s2 = "GTCGTGACTGGGAAAACCCTGG", "GTCGTGAT"
    rec = fx["fastq_r1"].splitlines()
    r1, r2 = [], []
    for k in range(0, len(rec) - 3, 4):
        name = rec[k].split()[0]
        for c in range(1 + (k // 4) % 3):
            umi = "".join(rnd.choice("ACGT") for _ in range(12))
            tail = "".join(rnd.choice("ACGT") for _ in range(40))
            read2 = s1 + umi[:6] + s2 + umi[6:] + tail
            r1 += [f"{name}_{c} 1:N:0:AAAA", rec[k + 1], "+", rec[k + 3]]
            r2 += [f"{name}_{c} 2:N:0:AAAA", read2, "+", "I" * len(read2)]
    return "\n".join(r1) + "\n", "\n".join(r2) + "\n"


# ---- the contract, brute force ----

def _calls(G: translate.GeneInfo, dcrs):
    """Per DCR the dict translate.cdr3_batch gives, or None where the reference raises (IndexError, ValueError)."""
    inp = {"command": "pipeline"}
    try:
        return translate.cdr3_batch(dcrs, translate.out_headers, inp, G)
    except (IndexError, ValueError):
        if len(dcrs) == 1:
            return [None]
        half = len(dcrs) // 2
        return _calls(G, dcrs[:half]) + _calls(G, dcrs[half:])


def expected_clonotypes(tab: dict, G: translate.GeneInfo):
    """(table, stats, clonotype_of) as nat.clonotypes gives them, from the contract: the members are the productive entries,
    a clonotype the members with equal (v_call, j_call, junction_aa); its row has the sum of the counts, the number of members
    and the member with the largest count (ties: the smallest rank); rows by duplicate_count descending, then that rank."""
    rows = table_rows(tab)
    recs = _calls(G, [[str(r[0]), str(r[1]), str(r[2]), str(r[3]), r[4]] for r in rows]) if rows else []
    stats = dict.fromkeys(nat.CLONOTYPE_STATS, 0)
    stats["entries_in"] = len(rows)
    groups = {}
    for k, (r, rec) in enumerate(zip(rows, recs)):
        stats["reads_in"] += r[5]
        kind = "untranslatable" if rec is None else "productive" if rec["productive"] == "T" else "nonproductive"
        stats[kind] += 1
        stats[kind + "_reads"] += r[5]
        if kind == "productive":
            groups.setdefault((rec["v_call"], rec["j_call"], rec["junction_aa"]), []).append(k)
    out = []
    for key, members in groups.items():
        rep = min(members, key=lambda k: (-rows[k][5], k))
        out.append((sum(rows[k][5] for k in members), rep, len(members), rows[rep][5], key, recs[rep]["junction"], members))
    out.sort(key=lambda x: (-x[0], x[1]))
    of = np.full(len(rows), nat.NOT_A_MEMBER, dtype=np.uint32)
    for r, x in enumerate(out):
        of[x[6]] = r
    stats["clonotypes_out"] = len(out)
    stats["convergent"] = sum(1 for x in out if x[2] > 1)
    stats["largest_n_dcrs"] = max((x[2] for x in out), default=0)
    tabl = {"rep": np.array([x[1] for x in out], dtype=np.uint32), "duplicate_count": np.array([x[0] for x in out], dtype=np.uint64),
            "n_dcrs": np.array([x[2] for x in out], dtype=np.uint32), "top_dcr_count": np.array([x[3] for x in out], dtype=np.uint64),
            "junction_aa": [x[4][2] for x in out], "junction": [x[5] for x in out], "v_call": [x[4][0] for x in out],
            "j_call": [x[4][1] for x in out]}
    return tabl, stats, of


def junctions(tabl: dict):
    """(junction_aa, junction) lists of a table nat.clonotypes gave."""
    off, text = tabl["junc_off"], tabl["junc_text"]
    cut = [text[int(off[k]):int(off[k + 1])].decode("latin-1") for k in range(len(off) - 1)]
    return cut[0::2], cut[1::2]


def brute_force_native(G: translate.GeneInfo):
    """What stands in for _native.clonotypes in the CPU tests of the stage: the brute force, in the native function's shape."""
    def clonotypes(genes, counted):
        tabl, stats, of = expected_clonotypes(counted, G)
        text, off = b"", [0]
        for a, b in zip(tabl["junction_aa"], tabl["junction"]):
            for s in (a, b):
                text += s.encode("latin-1")
                off.append(len(text))
        return dict(tabl, junc_off=np.array(off, dtype=np.uint64), junc_text=text), stats, of
    return clonotypes


def assert_same(got, want):
    """(table, stats, clonotype_of) of nat.clonotypes against expected_clonotypes: every array, exactly."""
    (gt, gs, gof), (wt, ws, wof) = got, want
    assert gs == ws, (gs, ws)
    for k in ("rep", "duplicate_count", "n_dcrs", "top_dcr_count"):
        assert gt[k].tolist() == wt[k].tolist(), k
    ja, jn = junctions(gt)
    assert ja == wt["junction_aa"] and jn == wt["junction"]
    assert np.array_equal(gof, wof)
    assert int(gt["duplicate_count"].sum()) == ws["productive_reads"]


def file_text(tabl_expected: dict, tab: dict) -> str:
    """The `.clonotypes.tsv` text of an expected table, written from the contract's column list."""
    rows = table_rows(tab)
    lines = ["\t".join(nat.CLONOTYPE_COLUMNS)]
    for r in range(len(tabl_expected["rep"])):
        e = rows[int(tabl_expected["rep"][r])]
        lines.append("\t".join([tabl_expected["v_call"][r], tabl_expected["j_call"][r], tabl_expected["junction_aa"][r],
                                str(int(tabl_expected["duplicate_count"][r])), str(int(tabl_expected["n_dcrs"][r])),
                                tabl_expected["junction"][r], ", ".join(str(x) for x in e[:5]),
                                str(int(tabl_expected["top_dcr_count"][r]))]))
    return "\n".join(lines) + "\n"


# ---- the per-entry code on the host (tests/host_clono) against dcrx_cdr3_batch ----

_host = None


def host_lib():
    global _host
    if _host is None:
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_clono")])
        _host = C.CDLL(HOST_LIB)
        _host.clono_host_calls.restype = C.c_int64
        _host.clono_host_calls.argtypes = [C.POINTER(nat.Cdr3GenesC)] + [C.c_void_p] * 2 + [C.c_uint64] + [C.c_void_p] * 8 + [C.c_uint64]
        _host.clono_host_key_equal.restype = C.c_int
        _host.clono_host_key_equal.argtypes = [C.POINTER(nat.Cdr3GenesC), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64,
                                               C.c_char_p, C.c_int32, C.c_int32, C.c_uint64, C.c_char_p]
    return _host


def host_calls(G: translate.GeneInfo, tab: dict):
    """(rows[CLONO_ROW_DTYPE], arena bytes) of the host build for a table."""
    genes = translate._native_genes(G)
    vg, jg = nat.call_groups(G.v_names), nat.call_groups(G.j_names)
    n = len(tab["v"])
    rows = np.zeros(n, dtype=nat.CLONO_ROW_DTYPE)
    text = np.frombuffer(tab["ins_text"] + b"\0", np.uint8)
    args = [C.byref(genes.c), vg.ctypes.data, jg.ctypes.data, n] + [tab[k].ctypes.data for k in ("v", "j", "vdel", "jdel", "ins_off")] + \
           [text.ctypes.data, rows.ctypes.data]
    need = host_lib().clono_host_calls(*args, None, 0)
    assert need >= 0
    arena = np.zeros(max(1, need), np.uint8)
    assert host_lib().clono_host_calls(*args, arena.ctypes.data, need) == need
    return rows, arena[:need].tobytes()


SHARED_FIELDS = ("status", "in_frame", "stop", "conserved_c", "conserved_f", "productive", "start_cdr3", "end_cdr3", "seq_len",
                 "aa_len", "bad_codon_at", "junction_aa_off", "junction_aa_len", "junction_off", "junction_len")


def assert_rows_equal_batch(G: translate.GeneInfo, tab: dict, rows, arena: bytes) -> dict:
    """rows / arena (the host build's or the device's) against dcrx_cdr3_batch on the same table: every shared field, and the
    junction bytes of the productive entries.  Returns how many rows had each status."""
    r = table_rows(tab)
    ref, text = nat.cdr3_batch(translate._native_genes(G), [x[0] for x in r], [x[1] for x in r], [x[2] for x in r], [x[3] for x in r],
                               [x[4] for x in r])
    nj = len(G.j_regions)
    j_pos = [G.j_translate_position[x[1] % nj] if -nj <= x[1] < nj else 0 for x in r]
    got = nat.clono_row_fields(rows, j_pos)
    # a row the reference raises on "keeps status != 0 and nothing else" (include/dcrx.h; bad_codon_at for BAD_CODON): whatever
    # else dcrx_cdr3_batch had filled in before it gave the row up is no part of its contract
    raised = (ref["status"] == nat.CDR3_INDEX_ERROR) | (ref["status"] == nat.CDR3_BAD_CODON)
    for f in SHARED_FIELDS:
        differs = got[f] != ref[f]
        if f not in ("status", "bad_codon_at"):
            differs &= ~raised
        bad = np.nonzero(differs)[0]
        assert len(bad) == 0, (f, int(bad[0]), r[int(bad[0])], int(got[f][bad[0]]), int(ref[f][bad[0]]))
    at = 0
    for k in range(len(r)):
        if ref[k]["status"] == nat.CDR3_OK and ref[k]["productive"]:
            assert int(rows[k]["arena_off"]) == at, k
            ja = text[int(ref[k]["aa_off"]) + int(ref[k]["junction_aa_off"]):][:int(ref[k]["junction_aa_len"])]
            jn = text[int(ref[k]["seq_off"]) + int(ref[k]["junction_off"]):][:int(ref[k]["junction_len"])]
            assert arena[at:at + len(ja) + len(jn)] == ja + jn, (k, r[k])
            at += len(ja) + len(jn)
    assert at == len(arena)
    return {s: int((ref["status"] == s).sum()) for s in range(4)}


# ---- the generators of tests/test_cdr3_native.py (random sequences with ambiguity codes, gaps, motif searches), as tables ----

def ambiguity_case(seed: int = 7):
    """Random V regions with IUPAC codes, lower case and U, translated whole (no J bases, no insert)."""
    rnd = random.Random(seed)
    letters = "ACGT" * 6 + "NRYKMSWBDHVXUacgtn"
    seqs = ["".join(rnd.choice(letters) for _ in range(rnd.randrange(0, 70))) for _ in range(400)]
    G = gene_info(seqs, [""], [1] * len(seqs), ["C"] * len(seqs), [0], ["FG.G"])
    return G, table([(k, 0, 0, 0, "", 1) for k in range(len(seqs))])


def ambiguous_insert_case(seed: int = 8):
    """The golden genes with inserts that hold IUPAC codes, lower case, U, gaps and letters that are no nucleotide code."""
    rnd = random.Random(seed)
    G = golden_genes()
    letters = "ACGT" * 8 + "NRYKMSWBDHVXUacgtnryk-J"
    rows = []
    for _ in range(600):
        ins = "".join(rnd.choice(letters) for _ in range(rnd.randrange(0, 12)))
        if rnd.random() < 0.1:
            ins += "---"
        rows.append((rnd.randrange(-8, 8), rnd.randrange(-5, 5), rnd.randrange(0, 12), rnd.randrange(0, 12), ins, 1))
    return G, table(rows)


def gap_case():
    G = gene_info(["TGT---GCA", "TGT-A-GCA"], [""], [1] * 2, ["C"] * 2, [0], ["A"])
    return G, table([(0, 0, 0, 0, "", 1), (1, 0, 0, 0, "", 1)])


def motif_cases(seed: int = 11):
    rnd = random.Random(seed)
    aas = "ACDEFGHIKLMNPQRSTVWY*X"
    for motif in ("FG.G", "[FW]G.G", "G", "[A-F][^G]", "..", "F\\*", "", "FGXGA", "(F|W)G.G", "FG.G?", "^FG", "\\w"):
        seqs = ["".join(rnd.choice("ACGT") for _ in range(rnd.randrange(30, 90))) for _ in range(150)]
        G = gene_info(seqs, ["", ""], [rnd.randrange(1, 8) for _ in seqs], [rnd.choice(aas) for _ in seqs], [-6, 2], [motif, motif])
        yield motif, G, table([(k, rnd.randrange(2), 0, 0, "", 1) for k in range(len(seqs))])


def golden_case_tables():
    """The 1 308 cases of translate_cdr3.json as two tables (the `translate` command's rows carry a blank in front of the
    insert, which the stage strips), with which of them the reference raised IndexError on."""
    fx = json.load(open(GOLDEN))
    out = []
    for command in ("pipeline", "translate"):
        cases = [c for c in fx["cases"] if c["command"] == command]
        rows = [(int(c["dcr"][0]), int(c["dcr"][1]), int(c["dcr"][2]), int(c["dcr"][3]),
                 c["dcr"][4][1:] if command == "translate" else c["dcr"][4], 1) for c in cases]
        out.append((table(rows), [c["expect"] == "IndexError" for c in cases], cases))
    return out


def coding_table():
    fx = json.load(open(CODING_FX))
    return translate.GeneInfo(**fx["genes"]), table([(int(d[0]), int(d[1]), int(d[2]), int(d[3]), d[4], 1) for d in fx["dcrs"]]), fx
