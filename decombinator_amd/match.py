"""The `match` sub-command: which of a sample's clonotypes are the same as, or one or two CDR3 residues from, an entry of a
second table — a list of CDR3s of known specificity (a VDJdb or McPAS export, a lab's sorted clones), or another sample.

    python -m decombinator_amd match -in A.clonotypes.tsv [B.clonotypes.tsv.gz ...] -db known.tsv[.gz] [-op DIR] [-pf dcr_] [-dz]
           [--cdr3-distance 0|1|2] [--cdr3-metric hamming|levenshtein] [--cdr3-class none|v|vj] [--strip-alleles]
           [--cdr3-metric weighted [--cdr3-radius N] [--cdr3-gap-cost N] [--cdr3-trim N,C] [--cdr3-cost-matrix FILE]]
           [--db-cdr3-column NAME] [--db-v-column NAME] [--db-j-column NAME]

The samples are 1 to 64 `.clonotypes.tsv` files (overlap.read_table; a sample is named as `overlap` names it).  The database is
any tab-separated table with a header line, its columns found by NAME (junction_aa, v_call, j_call by default: a
`.clonotypes.tsv` is a database as it stands, and `match -in A.clonotypes.tsv -db B.clonotypes.tsv` is near-match sharing
between two samples).  The database becomes ONE _native.Cdr3Index on the GPU, and every sample is ONE _native.cdr3_match
against it (include/dcrx.h "match").  The reference has no counterpart; there is no CPU fallback.

A hit joins a clonotype and a database entry of one class (--cdr3-class: nothing, the V call — the default, the network's —
or the V and the J call; numbered from the call STRINGS over the database and all samples, with --strip-alleles up to the
first `*` on both sides: no gene set and no -tfdir are needed) whose CDR3s are at most --cdr3-distance (default 1) apart under
--cdr3-metric (hamming, the default: substitutions between CDR3s of one length; levenshtein: insertions and deletions too).

--cdr3-metric weighted asks the field's usual question instead (include/dcrx.h "match, weighted"; _native.cdr3_match_weighted):
a TCRdist-style distance with a radius.  A substitution costs what the table says (--cdr3-cost-matrix; by default 3 * min(4, 4 -
BLOSUM62): 12 for most pairs, 3 for I-V), a length difference is ONE gap at the best place at --cdr3-gap-cost (12) a position, the
first N and last C residues of the shorter CDR3 (--cdr3-trim, 3,2) do not count, and a hit lies within --cdr3-radius (24).  Those
defaults follow TCRdist's CDR3 settings: a design choice, not a measured optimum.  --cdr3-distance does not apply.  A CDR3 with a
byte outside A..Z takes no part, and the stage prints how many it left out; the files' distance column holds the weighted distance.

Per sample `<prefix><sample>.cdr3_matches.tsv[.gz]`: one line per hit, ordered by (clonotype, target): clonotype (the 0-based
row of the sample's table), v_call, j_call, junction_aa, duplicate_count, target (the 0-based row of the database), distance,
then the database line's columns verbatim under their own names prefixed `db_`.  Once `<prefix>match_targets.tsv[.gz]`: one
line per database entry that any sample hit, in database order: target, its columns (`db_`...), and per sample
`<sample>_clonotypes` and `<sample>_reads` (the clonotypes that hit it, and the sum of their reads)."""
from __future__ import annotations

import gzip

import numpy as np

from . import _native as nat
from .overlap import read_table, sample_name

CLASSES = ("none", "v", "vj")
DB_COLUMNS = {"db_cdr3_column": "junction_aa", "db_v_column": "v_call", "db_j_column": "j_call"}

stats: dict = {}      # per sample name, the statistics of the last run()


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    files = list(inp.get("infile") or [])
    if not 1 <= len(files) <= nat.CDR3_MATCH_MAX_SAMPLES:
        return f"match takes 1 to {nat.CDR3_MATCH_MAX_SAMPLES} .clonotypes.tsv files (-in), not {len(files)}"
    names = [sample_name(f) for f in files]
    for k, name in enumerate(names):
        if name in names[:k]:
            return f"two files give one sample name ({name!r}): {files[names.index(name)]} and {files[k]}"
    if not inp.get("database"):
        return "match takes a database (-db): a tab-separated table with a header line"
    distance = inp.get("cdr3_distance", 1)
    if isinstance(distance, bool) or not isinstance(distance, int) or not 0 <= distance <= 2:
        return f"--cdr3-distance is 0, 1 or 2, not {distance!r}"
    if inp.get("cdr3_metric", "hamming") not in tuple(nat.CDR3_METRICS) + (WEIGHTED,):
        return f"--cdr3-metric is one of {', '.join(tuple(nat.CDR3_METRICS) + (WEIGHTED,))}, not {inp['cdr3_metric']}"
    why = weighted_refusal(inp)
    if why:
        return why
    if inp.get("cdr3_class", "v") not in CLASSES:
        return f"--cdr3-class is none, v or vj, not {inp['cdr3_class']}"
    return None


WEIGHTED = "weighted"
WEIGHTED_OPTIONS = {"cdr3_radius": "--cdr3-radius", "cdr3_gap_cost": "--cdr3-gap-cost", "cdr3_trim": "--cdr3-trim",
                    "cdr3_cost_matrix": "--cdr3-cost-matrix"}
WEIGHTED_DEFAULTS = {"cdr3_radius": 24, "cdr3_gap_cost": 12, "cdr3_trim": "3,2"}      # after TCRdist's CDR3 settings: a design choice


def parse_trim(text):
    """(N, C) of "N,C", or None."""
    parts = str(text).split(",")
    if len(parts) != 2 or not all(x.strip().isdigit() for x in parts):
        return None
    return int(parts[0]), int(parts[1])


def weighted_refusal(inp: dict):
    """What refusal() adds for the weighted metric and its options — decided before any file is opened."""
    given = [flag for key, flag in WEIGHTED_OPTIONS.items() if inp.get(key) is not None]
    if inp.get("cdr3_metric", "hamming") != WEIGHTED:
        return f"{given[0]} goes with --cdr3-metric weighted" if given else None
    if inp.get("cdr3_distance", 1) != 1:
        return "--cdr3-distance does not apply to --cdr3-metric weighted: the radius is --cdr3-radius"
    radius = inp.get("cdr3_radius") if inp.get("cdr3_radius") is not None else WEIGHTED_DEFAULTS["cdr3_radius"]
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= nat.CDR3_MAX_RADIUS:
        return f"--cdr3-radius is 0 to {nat.CDR3_MAX_RADIUS}, not {radius!r}"
    gap = inp.get("cdr3_gap_cost") if inp.get("cdr3_gap_cost") is not None else WEIGHTED_DEFAULTS["cdr3_gap_cost"]
    if isinstance(gap, bool) or not isinstance(gap, int) or not 1 <= gap <= nat.CDR3_COST_MAX_GAP:
        return f"--cdr3-gap-cost is 1 to {nat.CDR3_COST_MAX_GAP}, not {gap!r}"
    trim = parse_trim(inp.get("cdr3_trim") if inp.get("cdr3_trim") is not None else WEIGHTED_DEFAULTS["cdr3_trim"])
    if trim is None or max(trim) > nat.CDR3_COST_MAX_TRIM:
        return f"--cdr3-trim is N,C with 0 to {nat.CDR3_COST_MAX_TRIM} each, not {inp.get('cdr3_trim')!r}"
    return None


def weighted_settings(inp: dict):
    """(cost, radius) of arguments weighted_refusal() let pass; reads --cdr3-cost-matrix (ValueError by line for a bad one)."""
    get = lambda key: inp.get(key) if inp.get(key) is not None else WEIGHTED_DEFAULTS[key]
    ntrim, ctrim = parse_trim(get("cdr3_trim"))
    if inp.get("cdr3_cost_matrix"):
        cost = nat.Cdr3Cost.from_file(inp["cdr3_cost_matrix"], get("cdr3_gap_cost"), ntrim, ctrim)
    else:
        cost = nat.Cdr3Cost.default(get("cdr3_gap_cost"), ntrim, ctrim)
    return cost, get("cdr3_radius")


def letters_only(s: bytes) -> bool:
    return all(65 <= b <= 90 for b in s)


def call_key(call: str, strip_alleles: bool) -> str:
    """What of a call two sides must share: the call, or with --strip-alleles what stands before its first `*`."""
    return call.split("*", 1)[0] if strip_alleles else call


def class_key(mode: str, v: str, j: str, strip_alleles: bool):
    if mode == "none":
        return None
    if mode == "v":
        return call_key(v, strip_alleles)
    return (call_key(v, strip_alleles), call_key(j, strip_alleles))


def read_database(path: str, inp: dict) -> dict:
    """The database (plain or .gz): {"header": its column names (bytes), "lines": every entry's line verbatim (bytes, without
    its end), "cdr3": bytes per entry, "v", "j": str per entry ("" where the class does not need the column)}.  ValueError,
    after the header is read, for a named column the database lacks when the class (or the CDR3) needs it, and for a line with
    fewer fields than the header, by its number."""
    mode = inp.get("cdr3_class", "v")
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
    if not lines:
        raise ValueError(f"{path} has no header line")
    header = lines[0].split(b"\t")
    at = {}
    for option, needed in (("db_cdr3_column", True), ("db_v_column", mode in ("v", "vj")), ("db_j_column", mode == "vj")):
        name = inp.get(option) or DB_COLUMNS[option]
        if not needed:
            continue
        if name.encode("utf-8") not in header:
            raise ValueError(f"{path} has no column {name!r} (--{option.replace('_', '-')}); its columns are "
                             + ", ".join(h.decode("utf-8", "replace") for h in header))
        at[option] = header.index(name.encode("utf-8"))
    cdr3, v, j = [], [], []
    for n, line in enumerate(lines[1:], 2):
        f = line.split(b"\t")
        if len(f) < len(header):
            raise ValueError(f"{path}, line {n}: {len(f)} fields, fewer than the header's {len(header)}")
        cdr3.append(f[at["db_cdr3_column"]])
        v.append(f[at["db_v_column"]].decode("latin-1") if "db_v_column" in at else "")
        j.append(f[at["db_j_column"]].decode("latin-1") if "db_j_column" in at else "")
    return {"header": header, "lines": lines[1:], "cdr3": cdr3, "v": v, "j": j}


def spans(strings):
    """(off, text) of a list of byte strings."""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        off[1:] = np.cumsum([len(b) for b in strings])
    return off, b"".join(strings)


def targets_text(db: dict, names, per_sample) -> bytes:
    """The `match_targets.tsv` text: the database entries some sample hit, in database order, with per sample (t_queries,
    t_weight) of its result."""
    head = [b"target"] + [b"db_" + h for h in db["header"]]
    for name in names:
        enc = name.encode("utf-8", "surrogateescape")
        head += [enc + b"_clonotypes", enc + b"_reads"]
    out = [b"\t".join(head)]
    hit_any = np.zeros(len(db["lines"]), dtype=bool)
    for tq, _ in per_sample:
        hit_any |= np.asarray(tq) > 0
    for t in np.flatnonzero(hit_any).tolist():
        row = [str(t).encode(), db["lines"][t]]
        for tq, tw in per_sample:
            row += [str(int(tq[t])).encode(), str(int(tw[t])).encode()]
        out.append(b"\t".join(row))
    return b"\n".join(out) + b"\n"


def run(inp: dict) -> dict:
    """The stage: refusals, the database, its index, then per sample the one call, the statistics line and the file; the
    targets' file last.  Returns {"matches": [names], "targets": name, "results": [...], "stats": [...]}.  ValueError for what
    refusal() and read_database() name, for a file that is no clonotype table and for a sample whose duplicate counts add up to
    2^64 or more (by the file's name)."""
    from .io import write_out_match
    why = refusal(inp)
    if why:
        raise ValueError(why)
    files = list(inp["infile"])
    names = [sample_name(f) for f in files]
    mode, strip = inp.get("cdr3_class", "v"), bool(inp.get("strip_alleles"))
    distance, metric = int(inp.get("cdr3_distance", 1)), inp.get("cdr3_metric", "hamming")
    cost, radius = weighted_settings(inp) if metric == WEIGHTED else (None, None)      # (the matrix file: before the database)
    db = read_database(inp["database"], inp)
    class_no = {}
    t_classes = [class_no.setdefault(class_key(mode, v, j, strip), len(class_no)) for v, j in zip(db["v"], db["j"])]
    t_off, t_text = spans(db["cdr3"])
    db_header = b"\t".join(b"db_" + h for h in db["header"])
    out = {"matches": [], "results": [], "stats": []}
    per_sample = []
    stats.clear()
    index = nat.Cdr3Index(np.array(t_classes, dtype=np.uint32), t_off, t_text)
    try:
        for name, path in zip(names, files):
            v, j, aa, dup = read_table(path)
            classes = [class_no.setdefault(class_key(mode, a, b, strip), len(class_no)) for a, b in zip(v, j)]
            v_no, j_no = {}, {}
            v_idx = [v_no.setdefault(x, len(v_no)) for x in v]
            j_idx = [j_no.setdefault(x, len(j_no)) for x in j]
            off, text = spans(aa)
            if sum(dup) >= 1 << 64:      # (before the sample's device call; the library refuses the same)
                raise ValueError(f"{path}: the duplicate counts add up to 2^64 or more")
            weights = np.array(dup, dtype=np.uint64)
            cls_arr = np.array(classes, dtype=np.uint32)
            if cost is not None:
                result = nat.cdr3_match_weighted(index, cls_arr, off, text, weights, cost, radius)
                not_letters = lambda strings: sum(1 <= len(s) <= nat.CDR3NET_MAX_LEN and not letters_only(s) for s in strings)
                st = dict(result["stats"], queries_not_letters=not_letters(aa), targets_not_letters=not_letters(db["cdr3"]))
                how = f"weighted, radius {radius}, gap {cost.gap}, trim {cost.ntrim},{cost.ctrim}"
                left_out = (f", {st['queries_not_letters']:,} clonotypes and {st['targets_not_letters']:,} entries left out for a byte "
                            "outside A..Z")
            else:
                result = nat.cdr3_match(index, cls_arr, off, text, weights, distance, metric)
                st, how, left_out = result["stats"], f"{metric} {distance}", ""
            stats[name] = st
            print(f"Match of {name} against {st['targets']:,} database entries ({how}, class {mode}): {st['queries']:,} "
                  f"clonotypes, {st['queries_hit']:,} with a hit ({st['queries_hit_weight']:,} reads), {st['hits']:,} hits, "
                  f"{st['queries_out_of_reach']:,} clonotypes and {st['targets_out_of_reach']:,} entries out of reach{left_out}")
            text_out = nat.format_cdr3_matches(result, v_idx, j_idx, list(v_no), list(j_no), off, text, weights, t_off, t_text, db_header,
                                               db["lines"], metric if cost is None else cost)
            out["matches"].append(write_out_match(text_out, name + ".cdr3_matches.tsv", inp))
            out["results"].append(result)
            out["stats"].append(st)
            per_sample.append((result["t_queries"], result["t_weight"]))
    finally:
        index.close()
    out["targets"] = write_out_match(targets_text(db, names, per_sample), "match_targets.tsv", inp)
    return out
