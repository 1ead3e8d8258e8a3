"""What the clonotype tests share (`translate --clonotypes`, include/dcrx.h "clonotypes"): the contract as a brute force in
Python on top of translate.cdr3_batch, table and gene-set generators, the host build of the per-entry code
(tests/host_clono), and the comparison of its rows with dcrx_cdr3_batch's; the constructed junction geometry (small genes
listed as data, every deletion, inserts that complete codons across both edges) with a plain Python model that says which edge
a row sits on, and one sequence spelt as several DCRs (respelt twins)."""
import ctypes as C
import json
import os
import random
import re

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
        _host.clono_host_pyslice.restype = None
        _host.clono_host_pyslice.argtypes = [C.c_int64] * 3 + [C.POINTER(C.c_int64)] * 2
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


# ---- constructed junction geometry: small genes listed as data, every deletion, inserts that complete codons across both edges ----

_FGAG = "TTTGGAGCAGGAACC"        # F G A G T

# (region, position, residue): the translation starts at the V region's first base
GEOMETRY_V = [
    ("GCATGTGCCAGCAGTTTA", 2, "C"),       # 0  the conserved C inside V (A C A S S L)
    ("GCATGTGCTTCATAAGC", 2, "C"),        # 1  a stop in codon 4 of 5: vdel 0..2 keep it whole, vdel 3 leaves TA in front of the insert
    ("GCATGTGCAGATAGC", 2, "C"),          # 2  ..ATAG..: TAG at base 11, out of frame; whole codons never read it (A C A D S)
    ("GCATGTGCTTCAGJAGC", 2, "C"),        # 3  a letter that is no code in codon 4 of 5
    ("gcaugyGCNrayTTC", 2, "C"),          # 4  lower case, U, IUPAC codes: ugy -> C, GCN -> A, ray -> B
    ("gcaugyGCNrayTTC", 4, "B"),          # 5  ... with the ambiguous residue as the conserved one
    ("", 0, "G"),                         # 6  no bases; position 0: Python's index -1, the LAST residue, and start_cdr3 = -1
    ("T", -2, "G"),                       # 7  one base; a negative position (index -3)
    ("TG", 2, "G"),                       # 8  two bases; the position lands in the insert or in the J piece
    ("GCATGTGCCAGCAGTTTA", 2, "CA"),      # 9  a residue of two characters: never conserved
    ("GCATAAGCCAGC", 2, "*"),             # 10 the residue '*': conserved, and a stop
    ("GCATGTGCCAGC", 0, "T"),             # 11 position 0 behind a V region with bases
    ("TGT", 6, "G"),                      # 12 the conserved C's codon alone; a position behind it, in the J piece
]

# (region, position, motif): a productive sequence ends one base behind a whole codon, so in-frame J codons end at len - 2
GEOMETRY_J = [
    ("TAA" + _FGAG + "G", -5, "FG.G"),               # 0  a stop at base 0
    ("GTAATGGGGAGCAGGAACCG", -5, "[FW]G.G"),         # 1  a stop at base 1 (W G A G T behind it)
    ("ACTGA" + _FGAG + "G", -5, "FG.G"),             # 2  a stop at base 2
    (_FGAG[:-2] + "TGACC", -5, "G"),                 # 3  a stop near the end, out of the productive frame; a one-token motif
    (_FGAG[:12] + "JCCG", -5, "FG.G"),               # 4  a letter that is no code
    ("", -5, ""),                                    # 5  no bases; the empty motif (found in any window)
    ("G", -1, "."),                                  # 6  one base
    ("GG", -2, "G"),                                 # 7  two bases
    ("uuuggngcnggaacyg", -5, "[FW]G.G"),             # 8  lower case, U, IUPAC codes: the same F G A G T
    ("CA" + _FGAG + "G", -40, "FG.G"),               # 9  a position far in front: the window's start clamps to 0
    ("A" + _FGAG + "G", 40, ""),                     # 10 a position far behind: the window clamps to nothing
    ("GAAGC" + _FGAG + "G", -5, "FGAGT"),            # 11 five tokens: the search looks at four residues, never found
]

GEOMETRY_INSERTS = [
    "", "G", "GC", "GCA", "GCAG", "GCAGG", "GCAGGT", "GCAGGTA",             # lengths 0 .. 7
    "AGC", "AGCA", "GA",                                                    # TA|A, TA|G (above), T|GA: stops across the V / insert edge
    "CT", "CTA", "GCT", "GCTA", "GCTG",                                     # T|AA, TA|A, TG|A: stops across the insert / J edge
    "JGCA", "GJCA", "GCJA", "GCAJ",                                         # a letter that is no code, at every offset
    "n", "NNN", "ta", "uga", "-", "---", "A--",
    "TGTGCA" + _FGAG[:12],                                                  # an insert that spells C A F G A G itself
]


def _codon_residue(c: str, _cache={}):
    """One codon's residue as translate.translate_nt gives it, and '-' for a codon of three gaps (Bio.Seq.translate's rule);
    None for a letter that is no nucleotide code."""
    if c not in _cache:
        try:
            _cache[c] = "-" if c == "---" else translate.translate_nt(c)
        except ValueError:
            _cache[c] = None
    return _cache[c]


def pieces(G: translate.GeneInfo, r):
    """(V[:-vdel], insert, J[jdel:]) of a row as Python slices them; None for a gene index outside its list."""
    try:
        V, J = G.v_regions[r[0]], G.j_regions[r[1]]
    except IndexError:
        return None
    return (V if r[2] == 0 else V[:-r[2]]), str(r[4]), J[r[3]:]


def plain_call(G: translate.GeneInfo, r) -> dict:
    """The contract for one row in plain Python on the joined sequence: nothing of libdcrx on this side.  status, the four call
    flags, productive, start, and where each residue was read from in the clonotype step's terms (nv: codons wholly inside
    the V piece; fj: the first codon wholly inside the J piece)."""
    p = pieces(G, r)
    if p is None:
        return {"status": nat.CDR3_INDEX_ERROR}
    seq = "".join(p)
    sn, an = len(seq), len(seq) // 3
    res = [_codon_residue(seq[3 * i:3 * i + 3]) for i in range(an)]
    fj = (len(p[0]) + len(p[1]) + 2) // 3
    j_base = len(G.j_regions[r[1]]) - len(p[2]) + 3 * fj - len(p[0]) - len(p[1])       # the J region's base that codon fj starts at
    out = {"sn": sn, "an": an, "nv": len(p[0]) // 3, "fj": fj, "res": res, "j_base": j_base}
    if None in res:
        return dict(out, status=nat.CDR3_BAD_CODON, bad=res.index(None))
    aa = "".join(res)
    vi, ji = r[0] % len(G.v_regions), r[1] % len(G.j_regions)
    out.update(in_frame=(sn - 1) % 3 == 0, stop="*" in aa, stops=[i for i, x in enumerate(aa) if x == "*"])
    try:
        hit = aa[G.v_translate_position[vi] - 1] == G.v_translate_residue[vi]
    except IndexError:
        return dict(out, status=nat.CDR3_INDEX_ERROR)
    idx = G.v_translate_position[vi] - 1
    out["c_at"] = idx + an if idx < 0 else idx
    start = idx if hit else 0
    window = aa[start:][G.j_translate_position[ji]:G.j_translate_position[ji] + 4]
    found = bool(re.findall(G.j_translate_residue[ji], window))
    out.update(status=nat.CDR3_OK, conserved_c=hit, conserved_f=found, start=start, window=len(window),
               productive=out["in_frame"] and not out["stop"] and hit and found)
    if out["productive"]:
        end = len(aa[start:]) + G.j_translate_position[ji] + start + 1
        out.update(junction_aa=aa[start:end], junction=seq[start * 3:3 * end])
    return out


def _v_first(G: translate.GeneInfo, v: int):
    """(first stop, first invalid codon) of a V region's frame-0 translation; None where there is none."""
    V = G.v_regions[v]
    res = [_codon_residue(V[3 * i:3 * i + 3]) for i in range(len(V) // 3)]
    return (res.index("*") if "*" in res else None), (res.index(None) if None in res else None)


GEOMETRY_CLASSES = ("stop_straddling_only", "stop_j_table_only", "stop_v_last_codon", "v_stop_behind_stop_free", "v_stop_at_nv_stop_free",
                    "bad_v_last_codon", "v_bad_behind_no_bad", "v_bad_at_nv_no_bad", "bad_in_j", "bad_in_j_k0", "j_stop_cut_stop_free",
                    "vdel_past_v", "jdel_past_j", "c_direct", "c_direct_hit", "c_j_table", "c_j_table_hit", "c_v_last_codon",
                    "c_first_direct", "window_clamped", "start_negative")


def geometry_classes(G: translate.GeneInfo, r, ref) -> set:
    """Which edges of the clonotype step's index arithmetic a row sits on, from the row's pieces in Python (plain_call) and
    the dcrx_cdr3_batch row `ref` — never from the code under test.  Asserts that the two agree on the calls."""
    c = plain_call(G, r)
    assert c["status"] == int(ref["status"]), (r, c["status"], int(ref["status"]))
    out = set()
    if "sn" not in c:
        return out
    vi, ji = r[0] % len(G.v_regions), r[1] % len(G.j_regions)
    if r[2] > len(G.v_regions[vi]):
        out.add("vdel_past_v")
    if r[3] > len(G.j_regions[ji]):
        out.add("jdel_past_j")
    nv, fj, an = c["nv"], c["fj"], c["an"]
    v_stop, v_bad = _v_first(G, vi)
    if c["status"] == nat.CDR3_BAD_CODON:
        assert int(ref["bad_codon_at"]) == 3 * c["bad"], r
        if c["bad"] == nv - 1:
            out.add("bad_v_last_codon")
        if c["bad"] >= fj:
            out.add("bad_in_j")
            if c["j_base"] >= 3:
                out.add("bad_in_j_k0")
        return out
    if v_bad is not None and v_bad >= nv:
        out.add("v_bad_behind_no_bad")
        if v_bad == nv:
            out.add("v_bad_at_nv_no_bad")
    st = c["stops"]
    if st and all(nv <= i < fj for i in st):
        out.add("stop_straddling_only")
    if st and all(i >= fj for i in st):
        out.add("stop_j_table_only")
    if st == [nv - 1]:
        out.add("stop_v_last_codon")
    if not st and v_stop is not None and v_stop >= nv:
        out.add("v_stop_behind_stop_free")
        if v_stop == nv:
            out.add("v_stop_at_nv_stop_free")
    if not st and fj < an:
        # a stop in the J region in this phase in FRONT of the base the entry's first whole J codon starts at, none behind
        J, first = G.j_regions[ji], c["j_base"]
        if any(_codon_residue(J[b:b + 3]) == "*" for b in range(first % 3, first - 2, 3)):
            out.add("j_stop_cut_stop_free")
    if c["status"] == nat.CDR3_INDEX_ERROR:
        return out
    assert (bool(ref["in_frame"]), bool(ref["stop"]), bool(ref["conserved_c"])) == (c["in_frame"], c["stop"], c["conserved_c"]), r
    assert int(ref["start_cdr3"]) == c["start"], r
    if ref["status"] == nat.CDR3_OK:
        assert (bool(ref["conserved_f"]), bool(ref["productive"])) == (c["conserved_f"], c["productive"]), r
    at = c["c_at"]
    if nv <= at < fj:
        out.add("c_direct")
        if c["conserved_c"]:
            out.add("c_direct_hit")
        if at == nv:
            out.add("c_first_direct")
    elif at >= fj:
        out.add("c_j_table")
        if c["conserved_c"]:
            out.add("c_j_table_hit")
    elif at == nv - 1:
        out.add("c_v_last_codon")
    if c["window"] < 4:
        out.add("window_clamped")
    if int(ref["start_cdr3"]) < 0:
        out.add("start_negative")
    return out


def geometry_genes() -> translate.GeneInfo:
    G = gene_info([g[0] for g in GEOMETRY_V], [g[0] for g in GEOMETRY_J], [g[1] for g in GEOMETRY_V], [g[2] for g in GEOMETRY_V],
                  [g[1] for g in GEOMETRY_J], [g[2] for g in GEOMETRY_J])
    # the genes' premises
    tr = lambda s: [_codon_residue(s[i:i + 3]) for i in range(0, len(s) - 2, 3)]
    assert _v_first(G, 1) == (4, None) and len(G.v_regions[1]) // 3 == 5 and _v_first(G, 3) == (None, 4) and _v_first(G, 10)[0] == 1
    V = G.v_regions[2]
    assert "ATAG" in V and "*" not in tr(V) and "*" in tr(V[2:])                   # a stop no whole frame-0 codon reads
    assert "".join(tr(G.v_regions[4])) == "ACABF" and sorted(len(v) for v in G.v_regions)[:3] == [0, 1, 2]
    assert [tr(G.j_regions[k][k:])[0] for k in range(3)] == ["*"] * 3              # a stop in each phase at the front
    assert all("*" not in tr(G.j_regions[k][k + 3:]) for k in range(3))
    J = G.j_regions[3]
    assert "*" not in tr(J[(len(J) - 1) % 3:]) and tr(J[1:])[-1] == "*"              # near the end, out of the productive frame
    assert None in tr(G.j_regions[4]) and sorted(len(j) for j in G.j_regions)[:3] == [0, 1, 2]
    assert "".join(tr(G.j_regions[8])) == "FGAGT"
    return G


def geometry_rows(G: translate.GeneInfo, inserts=GEOMETRY_INSERTS):
    """Every V with every J, every vdel in -2 .. len(V) + 2, every jdel in -2 .. len(J) + 2, every insert; then the gene indices
    on the lists' edges (-1, -n, -n - 1, n) on both sides."""
    nv, nj = len(G.v_regions), len(G.j_regions)
    for v in range(nv):
        for j in range(nj):
            for vdel in range(-2, len(G.v_regions[v]) + 3):
                for jdel in range(-2, len(G.j_regions[j]) + 3):
                    for ins in inserts:
                        yield (v, j, vdel, jdel, ins, 1)
    for v in (-1, -nv, -nv - 1, nv):
        for j in (-1, -nj, -nj - 1, nj, 0):
            for ins in ("", "GCA", "GCAG"):
                yield (v, j, 1, 1, ins, 1)
    for j in (-1, -nj, -nj - 1, nj):
        for ins in ("", "GCA", "GCAG"):
            yield (0, j, 1, 1, ins, 1)


GEOMETRY_STRIDE = 11      # the thinned list keeps one row in 11: coprime to the 28 inserts and to the deletion ranges


def geometry_case(thin: bool = False):
    """(genes, table) of the constructed junction geometry: the full product (about 1.15 M rows), or thinned to every
    GEOMETRY_STRIDE-th row of it (all the edge gene indices kept)."""
    G = geometry_genes()
    rows = list(geometry_rows(G))
    if thin:
        edge = [r for r in rows if not (0 <= r[0] < len(G.v_regions) and 0 <= r[1] < len(G.j_regions))]
        rows = rows[:len(rows) - len(edge)][::GEOMETRY_STRIDE] + edge
    return G, table(rows)


def batch_rows(G: translate.GeneInfo, tab: dict):
    r = table_rows(tab)
    return r, nat.cdr3_batch(translate._native_genes(G), [x[0] for x in r], [x[1] for x in r], [x[2] for x in r], [x[3] for x in r],
                             [x[4] for x in r])[0]


def geometry_premises(G: translate.GeneInfo, tab: dict) -> dict:
    """The premises of a geometry list, counted on dcrx_cdr3_batch's rows and the plain Python model: rows per status, the
    combinations of the four call flags, the productive rows, rows per edge class (GEOMETRY_CLASSES).  Asserts the floors."""
    r, ref = batch_rows(G, tab)
    n = {"status": {s: int((ref["status"] == s).sum()) for s in range(4)}}
    ok = ref["status"] == nat.CDR3_OK
    n["flag_combinations"] = len(set(zip(*(ref[f][ok].tolist() for f in ("in_frame", "stop", "conserved_c", "conserved_f")))))
    n["productive"] = int(ref["productive"][ok].sum())
    n["classes"] = dict.fromkeys(GEOMETRY_CLASSES, 0)
    for x, y in zip(r, ref):
        for c in geometry_classes(G, x, y):
            n["classes"][c] += 1
    assert all(n["status"][s] >= 1000 for s in (nat.CDR3_OK, nat.CDR3_INDEX_ERROR, nat.CDR3_BAD_CODON)), n
    assert n["flag_combinations"] == 16 and n["productive"] >= 500, n
    assert all(k >= 20 for k in n["classes"].values()), n
    return n


# ---- one sequence spelt as several DCRs ----

def respelt_twins(G: translate.GeneInfo, rows, v_moves=(1, 2, 3, 4, 5), j_moves=(1, 2, 3, 4, 5)) -> list:
    """Per base row (v, j, vdel, jdel, insert, ...) with both deletions inside their genes, the list of its spellings: the base,
    k bases moved from the end of V[:vend] into the front of the insert (vdel + k), k bases moved from the front of the J piece
    onto the insert's end (jdel + k), and both at once (equal k), as far as the pieces have the bases.  A base whose spellings
    meet an earlier base's is left out.  Premise: every spelling joins to the base's sequence."""
    sets, seen = [], set()
    for r in rows:
        v, j, vdel, jdel, ins = r[:5]
        V, J = G.v_regions[v], G.j_regions[j]
        if not (0 <= v < len(G.v_regions) and 0 <= j < len(G.j_regions) and 0 <= vdel <= len(V) and 0 <= jdel <= len(J)):
            continue
        vend = len(V) - vdel
        forms = [(v, j, vdel, jdel, ins)]
        moves = [(k, 0) for k in v_moves] + [(0, k) for k in j_moves] + [(k, k) for k in v_moves if k in j_moves]
        for kv, kj in moves:
            if kv <= vend and kj <= len(J) - jdel:
                forms.append((v, j, vdel + kv, jdel + kj, V[vend - kv:vend] + ins + J[jdel:jdel + kj]))
        if len(forms) < 2 or seen & set(forms):
            continue
        seen |= set(forms)
        assert len(set(forms)) == len(forms) and len({"".join(pieces(G, f)) for f in forms}) == 1, r
        sets.append(forms)
    return sets


def twin_table(sets, first_count: int = 1):
    """The spellings of `sets` as one table, set after set, every row with a count of its own; and per set its row numbers."""
    rows, where = [], []
    for forms in sets:
        where.append(list(range(len(rows), len(rows) + len(forms))))
        rows += [f + (first_count + len(rows) + k,) for k, f in enumerate(forms)]
    return table(rows), where


def assert_twins_agree(rows, arena: bytes, where) -> int:
    """Within every twin set the primitive's rows are one answer: status, flags, start_cdr3 (for a BAD_CODON row 3 x the codon),
    end_cdr3, seq_len, hash and the junction bytes.  Returns how many sets are productive."""
    f = nat.clono_row_fields(rows)
    productive = 0
    for ks in where:
        a = ks[0]
        span = lambda k: arena[int(rows[k]["arena_off"]):int(rows[k]["arena_off"]) + int(f[k]["junction_aa_len"]) + int(f[k]["junction_len"])]
        for k in ks[1:]:
            for name in ("status", "flags", "start_cdr3", "end_cdr3", "seq_len", "hash"):
                assert rows[k][name] == rows[a][name], (name, a, k, int(rows[a][name]), int(rows[k][name]))
            assert span(k) == span(a), (a, k)
        productive += int(rows[a]["status"] == nat.CDR3_OK and rows[a]["flags"] & 1)
    return productive


def assert_twin_sets_share_a_clonotype(want, where) -> int:
    """On an expected result: every twin set is wholly in one clonotype (with n_dcrs >= its size) or wholly outside.  Returns
    how many are inside."""
    tabl, _, of = want
    inside = 0
    for ks in where:
        c = {int(of[k]) for k in ks}
        assert len(c) == 1, ks
        c = c.pop()
        if c != nat.NOT_A_MEMBER:
            assert int(tabl["n_dcrs"][c]) >= len(ks)
            inside += 1
    return inside


def geometry_twins(n_productive: int = 150, n_other: int = 250):
    """(genes, twin sets) over the geometry genes: bases taken from the thinned list, the first n_productive productive rows
    whose deletions lie inside their genes and n_other of the rest at an even stride."""
    G, tab = geometry_case(thin=True)
    r, ref = batch_rows(G, tab)
    inside = [k for k, x in enumerate(r) if 0 <= x[0] < len(G.v_regions) and 0 <= x[1] < len(G.j_regions)
              and 0 <= x[2] <= len(G.v_regions[x[0]]) and 0 <= x[3] <= len(G.j_regions[x[1]])]
    prod = [k for k in inside if ref[k]["status"] == nat.CDR3_OK and ref[k]["productive"]]
    prod = prod[::max(1, len(prod) // n_productive)][:n_productive]
    rest = [k for k in inside if not ref[k]["productive"]]
    rest = rest[::max(1, len(rest) // n_other)][:n_other]
    return G, respelt_twins(G, [r[k] for k in sorted(prod + rest)])


def coding_twins(n: int = 300, seed: int = 21):
    """(genes, twin sets) over coding_genes(3): n productive bases (whole V and J, inserts of whole sense codons), respelt
    with 1 .. 5 bases moved on either side and with 12 .. 17 V bases moved — the conserved C's codon ends 12 to 14 bases before
    the V region's end, so those spellings read the C, whole or in part, from the insert."""
    G = coding_genes(3)
    rnd = random.Random(seed)
    bases, seen = [], set()
    while len(bases) < n:
        v, j = rnd.randrange(len(G.v_regions)), rnd.randrange(len(G.j_regions))
        ins = coding_insert(G, v, j, "".join(rnd.choice(_SENSE) for _ in range(rnd.randrange(1, 5))))
        if (v, j, ins) not in seen:
            seen.add((v, j, ins))
            bases.append((v, j, 0, 0, ins))
    sets = respelt_twins(G, bases, v_moves=(1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17))
    c_end = [3 * G.v_translate_position[v] for v in range(len(G.v_regions))]
    assert all(any(len(G.v_regions[f[0]]) - f[2] < c_end[f[0]] - 2 for f in s) for s in sets)       # the C's codon wholly in the insert
    assert all(any(c_end[f[0]] - 2 <= len(G.v_regions[f[0]]) - f[2] < c_end[f[0]] for f in s) for s in sets)      # ... and straddling
    return G, sets


def sample_agrees_with_python_calls(G: translate.GeneInfo, tab: dict, every: int) -> int:
    """On every `every`-th row: dcrx_cdr3_batch's row against translate.cdr3_batch's record (through _calls: None where it
    raises) and against plain_call's, which joins and translates the sequence in Python.  Returns how many rows were looked at."""
    r, ref = batch_rows(G, tab)
    ks = list(range(0, len(r), every))
    recs = _calls(G, [[str(r[k][0]), str(r[k][1]), str(r[k][2]), str(r[k][3]), r[k][4]] for k in ks])
    for k, rec in zip(ks, recs):
        c = plain_call(G, r[k])
        assert (rec is None) == (c["status"] != nat.CDR3_OK) == (ref[k]["status"] != nat.CDR3_OK), r[k]
        if rec is None:
            continue
        flag = lambda b: "FT"[bool(b)]
        assert (rec["productive"], rec["vj_in_frame"], rec["stop_codon"], rec["conserved_c"], rec["conserved_f"]) == \
               tuple(flag(c[f]) for f in ("productive", "in_frame", "stop", "conserved_c", "conserved_f")), r[k]
        assert rec["sequence"] == "".join(pieces(G, r[k])) and rec["sequence_aa"] == "".join(c["res"]), r[k]
        assert (rec["junction_aa"], rec["junction"]) == (c.get("junction_aa", ""), c.get("junction", "")), r[k]
    return len(ks)


def mixed_block_table(n: int):
    """n rows of mixed geometry for the block edges: spellings of coding_twins() sets dealt round-robin (a set's members lie a
    whole round apart), every third row a non-member in turn — a stop in frame, a letter that is no code, out of frame — and
    every row with a count of its own.  Returns (genes, table, row numbers per twin set)."""
    G, sets = coding_twins(n=40, seed=22)
    sets = [s[:6] + s[-3:] for s in sets]                     # the short moves and the ones past the conserved C
    members = [(k, f) for depth in range(max(len(s) for s in sets)) for k, s in enumerate(sets) if depth < len(s) for f in [s[depth]]]
    rows, where, m = [], {}, 0
    for at in range(n):
        if at % 3 == 2:
            v, j = at % len(G.v_regions), at % len(G.j_regions)
            body = ("TAA" + "GCA" * (at // 40), "GCJ" + "GCA" * (at // 40), "GCAG" + "GCA" * (at // 40))[at // 3 % 3]
            rows.append((v, j, 0, 0, coding_insert(G, v, j, body), 1000 + at))
        else:
            k, f = members[m]
            m += 1
            where.setdefault(k, []).append(at)
            rows.append(f + (1000 + at,))
    return G, table(rows), [ks for ks in where.values() if len(ks) > 1]
