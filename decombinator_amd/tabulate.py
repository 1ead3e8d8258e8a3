"""The `tabulate` sub-command: count meta-clonotypes — (centroid CDR3, class, radius), as `metaclonotypes` writes them — in bulk
samples: per meta-clonotype and sample, how many clonotypes and how many reads fall inside the meta-clonotype's OWN radius —
tcrdist3's bulk tabulation, the table association tests are run on.

    python -m decombinator_amd tabulate -mc A.cdr3_metaclonotypes.tsv[.gz] -in S1.clonotypes.tsv [S2.clonotypes.tsv.gz ...]
           [-op DIR] [-pf dcr_] [-dz] [--mc-cdr3-column junction_aa] [--mc-v-column v_call] [--mc-j-column j_call]
           [--mc-radius-column radius] [--cdr3-class none|v|vj] [--strip-alleles] [--cdr3-gap-cost 12] [--cdr3-trim 3,2]
           [--cdr3-cost-matrix FILE]

The meta-clonotypes (-mc) are read as `match` reads its database (match.read_database: any tab-separated table with a header
line, its columns found by name); the defaults are the columns `metaclonotypes` writes, so its file goes in as it stands.  A row
whose radius is `.` is left out and counted; any other radius that is no integer 0 .. 65535 is a ValueError naming the line.  The
rows with a radius become ONE _native.Cdr3Index on the GPU, and each of the 1 to 64 samples (overlap.read_table; named as
`overlap` names them) is ONE _native.cdr3_tally_weighted call against it (include/dcrx.h "tally, weighted": one walk with a
radius per target that leaves totals per target — no hit list).  The reference has no counterpart; there is no CPU fallback.

The distance, the classes (numbered from the call STRINGS over -mc and all samples), the cost and who takes part (1 .. 32 letters
A..Z) are `match --cdr3-metric weighted`'s.  THE COST (--cdr3-gap-cost, --cdr3-trim, --cdr3-cost-matrix), --cdr3-class AND
--strip-alleles HAVE TO BE THE ONES THE META-CLONOTYPES WERE MADE UNDER: a radius means nothing under another distance.

`<prefix>tabulate.tsv[.gz]`: one line per meta-clonotype with a radius, in file order, rows of all zeros kept (an association
test needs them): metaclonotype (the 0-based data row of -mc), v_call, j_call, junction_aa, radius, samples (how many samples
hold a clonotype inside it), then per sample <sample>_clonotypes and <sample>_reads.  A centroid that takes no part (a byte
outside A..Z, or out of reach) keeps its line, with zeros.
`<prefix>tabulate_samples.tsv[.gz]`: per sample: sample, clonotypes, reads (the totals, for normalising), take_part,
clonotypes_inside and reads_inside (the clonotypes inside ANY meta-clonotype, each counted once), metaclonotypes_found."""
from __future__ import annotations

import numpy as np

from . import _native as nat
from .match import CLASSES, class_key, letters_only, read_database, spans, weighted_refusal, weighted_settings
from .overlap import read_table, sample_name

MAX_SAMPLES = nat.CDR3_TALLY_MAX_SAMPLES
MC_COLUMNS = {"mc_cdr3_column": "db_cdr3_column", "mc_v_column": "db_v_column", "mc_j_column": "db_j_column"}
MC_DEFAULTS = {"mc_cdr3_column": "junction_aa", "mc_v_column": "v_call", "mc_j_column": "j_call", "mc_radius_column": "radius"}
COLUMNS = ["metaclonotype", "v_call", "j_call", "junction_aa", "radius", "samples"]
SAMPLE_COLUMNS = ["sample", "clonotypes", "reads", "take_part", "clonotypes_inside", "reads_inside", "metaclonotypes_found"]

stats: dict = {}      # per sample name, the statistics of the last run()


def weighted_inp(inp: dict) -> dict:
    """The arguments as match's weighted routines read them: the metric is the weighted one; the radii are the file's."""
    return dict(inp, cdr3_metric="weighted", cdr3_distance=1, cdr3_radius=None)


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    files = list(inp.get("infile") or [])
    if not 1 <= len(files) <= MAX_SAMPLES:
        return f"tabulate takes 1 to {MAX_SAMPLES} .clonotypes.tsv files (-in), not {len(files)}"
    names = [sample_name(f) for f in files]
    for k, name in enumerate(names):
        if name in names[:k]:
            return f"two files give one sample name ({name!r}): {files[names.index(name)]} and {files[k]}"
    if not inp.get("metaclonotypes"):
        return "tabulate takes the meta-clonotypes (-mc): a tab-separated table with a header line, as `metaclonotypes` writes it"
    why = weighted_refusal(weighted_inp(inp))
    if why:
        return why
    if inp.get("cdr3_class", "v") not in CLASSES:
        return f"--cdr3-class is none, v or vj, not {inp['cdr3_class']}"
    return None


def takes_part(s: bytes) -> bool:
    return 1 <= len(s) <= nat.CDR3NET_MAX_LEN and letters_only(s)


def read_metaclonotypes(inp: dict) -> dict:
    """The meta-clonotypes through match.read_database, with the --mc-* columns in the --db-* columns' place: {"row": the 0-based
    data rows that have a radius, "v", "j" (str; for the class), "v_out", "j_out" (bytes; the file's columns where it has them),
    "cdr3" (bytes), "radius" (int) per such row, "rows": all data rows, "without_radius": those with `.`}."""
    path = inp["metaclonotypes"]
    as_db = {"cdr3_class": inp.get("cdr3_class", "v")}
    for mc, db in MC_COLUMNS.items():
        as_db[db] = inp.get(mc)
    try:
        db = read_database(path, as_db)
    except ValueError as e:
        raise ValueError(str(e).replace("--db-", "--mc-")) from None
    header = db["header"]
    name = inp.get("mc_radius_column") or MC_DEFAULTS["mc_radius_column"]
    if name.encode("utf-8") not in header:
        raise ValueError(f"{path} has no column {name!r} (--mc-radius-column); its columns are "
                         + ", ".join(h.decode("utf-8", "replace") for h in header))
    at_r = header.index(name.encode("utf-8"))
    shown = []
    for key in ("mc_v_column", "mc_j_column"):
        col = (inp.get(key) or MC_DEFAULTS[key]).encode("utf-8")
        shown.append(header.index(col) if col in header else None)
    out = {"row": [], "v": [], "j": [], "v_out": [], "j_out": [], "cdr3": [], "radius": [], "rows": len(db["lines"]), "without_radius": 0}
    for k, line in enumerate(db["lines"]):
        f = line.split(b"\t")
        cell = f[at_r].strip()
        if cell == b".":
            out["without_radius"] += 1
            continue
        if not cell.isdigit() or int(cell) > nat.CDR3_MAX_RADIUS:
            raise ValueError(f"{path}, line {k + 2}: the radius {cell.decode('latin-1')!r} is not an integer 0..{nat.CDR3_MAX_RADIUS} or `.`")
        out["row"].append(k); out["v"].append(db["v"][k]); out["j"].append(db["j"][k]); out["cdr3"].append(db["cdr3"][k])
        out["v_out"].append(f[shown[0]] if shown[0] is not None else b""); out["j_out"].append(f[shown[1]] if shown[1] is not None else b"")
        out["radius"].append(int(cell))
    return out


def table_text(mc: dict, names, results) -> bytes:
    head = COLUMNS + [f"{name}_{what}" for name in names for what in ("clonotypes", "reads")]
    out = ["\t".join(head).encode()]
    for k, row in enumerate(mc["row"]):
        cells = [str(row).encode(), mc["v_out"][k], mc["j_out"][k], mc["cdr3"][k], str(mc["radius"][k]).encode(),
                 str(sum(int(r["t_count"][k]) > 0 for r in results)).encode()]
        for r in results:
            cells += [str(int(r["t_count"][k])).encode(), str(int(r["t_weight"][k])).encode()]
        out.append(b"\t".join(cells))
    return b"\n".join(out) + b"\n"


def samples_text(names, per_sample) -> bytes:
    out = ["\t".join(SAMPLE_COLUMNS).encode()]
    for name, st in zip(names, per_sample):
        out.append("\t".join([name] + [str(st[c]) for c in SAMPLE_COLUMNS[1:]]).encode())
    return b"\n".join(out) + b"\n"


def run(inp: dict) -> dict:
    """The stage: refusals, the cost, the meta-clonotypes and their index, then per sample one tally and the printed line, and
    the two files.  Returns {"tabulate": name, "samples": name, "results": [...], "stats": [...]}.  ValueError for what
    refusal(), read_metaclonotypes() and match.weighted_settings() name and for a file that is no clonotype table."""
    from .io import write_out_tabulate
    why = refusal(inp)
    if why:
        raise ValueError(why)
    files = list(inp["infile"])
    names = [sample_name(f) for f in files]
    mode, strip = inp.get("cdr3_class", "v"), bool(inp.get("strip_alleles"))
    cost, _ = weighted_settings(weighted_inp(inp))      # (the matrix file: before the meta-clonotypes)
    mc = read_metaclonotypes(inp)
    class_no = {}
    t_classes = [class_no.setdefault(class_key(mode, v, j, strip), len(class_no)) for v, j in zip(mc["v"], mc["j"])]
    t_off, t_text = spans(mc["cdr3"])
    radii = np.array(mc["radius"], dtype=np.uint32)
    no_part = sum(not takes_part(s) for s in mc["cdr3"])
    out = {"results": [], "stats": []}
    stats.clear()
    index = nat.Cdr3Index(np.array(t_classes, dtype=np.uint32), t_off, t_text)
    try:
        for name, path in zip(names, files):
            v, j, aa, dup = read_table(path)
            classes = np.array([class_no.setdefault(class_key(mode, a, b, strip), len(class_no)) for a, b in zip(v, j)], dtype=np.uint32)
            off, text = spans(aa)
            result = nat.cdr3_tally_weighted(index, classes, off, text, np.array(dup, dtype=np.uint64), cost, radii)
            rs = result["stats"]
            st = {"clonotypes": len(aa), "reads": int(sum(dup)),
                  "take_part": len(aa) - rs["queries_out_of_reach"] - rs["queries_not_letters"], "clonotypes_inside": rs["queries_hit"],
                  "reads_inside": rs["queries_hit_weight"], "metaclonotypes_found": rs["targets_hit"]}
            stats[name] = st
            print(f"Tabulated {name} against {len(mc['row']):,} meta-clonotypes ({mc['without_radius']:,} more left out without a radius, "
                  f"{no_part:,} centroids take no part; gap {cost.gap}, trim {cost.ntrim},{cost.ctrim}, class {mode}): "
                  f"{st['clonotypes']:,} clonotypes, {st['reads']:,} reads, {st['take_part']:,} take part, {st['clonotypes_inside']:,} "
                  f"clonotypes with {st['reads_inside']:,} reads inside a meta-clonotype, {st['metaclonotypes_found']:,} meta-clonotypes found")
            out["results"].append(result)
            out["stats"].append(st)
    finally:
        index.close()
    out["tabulate"] = write_out_tabulate(table_text(mc, names, out["results"]), "tabulate.tsv", inp)
    out["samples"] = write_out_tabulate(samples_text(names, out["stats"]), "tabulate_samples.tsv", inp)
    return out
