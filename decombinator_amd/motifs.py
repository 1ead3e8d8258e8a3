"""The `motifs` sub-command: which short motifs — 2-, 3- and 4-mers in the hypervariable middle of the CDR3 — occur in more of a
sample's CDR3s than in as many CDR3s drawn from a background repertoire (GLIPH's "local" question, beside the "global" one
`match` and `--cdr3-network` answer).

    python -m decombinator_amd motifs -in A.clonotypes.tsv [B.clonotypes.tsv.gz ...] -bg naive.clonotypes.tsv[.gz]
           [--bg-cdr3-column junction_aa] [--motif-k 2,3,4] [--motif-trim 3,3] [--motif-min-count 3]
           [--resamples 1000] [--seed 1] [-op DIR] [-pf dcr_] [-dz]
           [--groups [--group-p-value 0.001] [--group-min-fold 10] [--group-distance 1] [--write-motif-members]]

The samples are 1 to 64 `.clonotypes.tsv` files (overlap.read_table; a sample is named as `overlap` names it).  The background
is any tab-separated table with a header line, its CDR3 column found by name (match.read_database's reading rules: another
sample's `.clonotypes.tsv` is a background as it stands).  A table's UNITS are its distinct junction_aa strings in order of first
appearance (a Python dict here on the host); every sample is ONE _native.cdr3_motifs against the background's units
(include/dcrx.h "motifs").  The reference has no counterpart; there is no CPU fallback.

A unit takes part when it has 1 to 32 bytes, all A..Z; the others are counted and the stage prints how many it left out.  A
motif of k letters (--motif-k) is looked for in the windows that leave out the first N and last C residues (--motif-trim; 3,3
after GLIPH: a design choice, not a measured optimum), once per unit.  Reported are the motifs in at least --motif-min-count (3: a
design choice) of the sample's units.  --resamples times as many background units as the sample has are drawn without
replacement (the key of `overlap --downsample`, seeded by --seed: the same seed gives the same files), and a motif's count in
every draw is compared with its count in the sample.

Per sample `<prefix><sample>.cdr3_motifs.tsv[.gz]`: one line per reported motif, ordered by resamples_at_least ascending, cdr3s
descending, k, motif: motif, k, cdr3s (the sample's units that hold it), background_cdr3s, resamples, resamples_at_least (the
draws that held it at least as often as the sample), resample_sum, resample_max, expected (resample_sum / resamples), fold
(cdr3s * resamples / resample_sum) and p_value ((resamples_at_least + 1) / (resamples + 1)); the last three exact fractions
at six decimals, `nan` on a zero denominator.

With --groups the sample's CDR3s are merged into GLIPH-style specificity groups (include/dcrx.h "motif groups"; ONE
_native.cdr3_motif_groups per sample).  A motif is SELECTED when its p_value is at most --group-p-value and its fold at least
--group-min-fold (a zero resample_sum passes), both compared as exact fractions of the flags' own text; 0.001 and 10 follow
GLIPH and are design choices, not measured optima.  Two CDR3s are linked when both hold one selected motif, or when they have one
length and differ in at most --group-distance residues (1 after GLIPH, a design choice; 0: no such links; any residue may
differ, not only the untrimmed middle, and V genes are not looked at); a group is a connected component.
`<prefix><sample>.cdr3_groups.tsv[.gz]` has one line per distinct CDR3 in order of first appearance: junction_aa, clonotypes
(the table rows with it), duplicate_count (their reads), group (numbered from 0 by first appearance, as `cluster` in
`.cdr3_clusters.tsv`), group_cdr3s, group_duplicate_count, degree (its links of the second kind) and motifs (its selected
motifs in motif order, comma-joined, `.` for none).  With --write-motif-members `<prefix><sample>.cdr3_motif_members.tsv[.gz]`
lists, per selected motif in motif order, the CDR3s that hold it: motif, k, junction_aa, position (of the first window that
holds it, 0-based from the CDR3's start) and group."""
from __future__ import annotations

import re
from fractions import Fraction

import numpy as np

from . import _native as nat
from .match import letters_only, parse_trim, read_database, spans
from .overlap import index_fraction, read_table, sample_name

DEFAULTS = {"motif_k": "2,3,4", "motif_trim": "3,3", "motif_min_count": 3, "resamples": 1000, "seed": 1,      # design choices (3,3 and 3 after GLIPH)
            "group_p_value": "0.001", "group_min_fold": "10", "group_distance": 1}      # ... as these are (after GLIPH)
GROUP_FLAGS = (("--group-p-value", "group_p_value"), ("--group-min-fold", "group_min_fold"), ("--group-distance", "group_distance"),
               ("--write-motif-members", "write_motif_members"))

stats: dict = {}      # per sample name, the statistics of the last run()


def parse_ks(text):
    """The sorted k of "2,3,4", or None."""
    parts = [x.strip() for x in str(text).split(",")]
    if not parts or not all(x.isdigit() and int(x) in nat.CDR3_MOTIF_KS for x in parts) or len(set(parts)) != len(parts):
        return None
    return sorted(int(x) for x in parts)


def _get(inp: dict, key: str):
    return inp.get(key) if inp.get(key) is not None else DEFAULTS[key]


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def parse_decimal(text):
    """The exact value of a decimal such as "0.001", "10" or ".5", or None."""
    text = str(text).strip()
    return Fraction(text) if re.fullmatch(r"[0-9]+(\.[0-9]*)?|\.[0-9]+", text) else None


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    files = list(inp.get("infile") or [])
    if not 1 <= len(files) <= nat.CDR3_MOTIF_MAX_SAMPLES:
        return f"motifs takes 1 to {nat.CDR3_MOTIF_MAX_SAMPLES} .clonotypes.tsv files (-in), not {len(files)}"
    names = [sample_name(f) for f in files]
    for k, name in enumerate(names):
        if name in names[:k]:
            return f"two files give one sample name ({name!r}): {files[names.index(name)]} and {files[k]}"
    if not inp.get("background"):
        return "motifs takes a background (-bg): a tab-separated table with a header line"
    if parse_ks(_get(inp, "motif_k")) is None:
        return f"--motif-k is a comma-separated list of distinct k out of 2, 3, 4, not {inp.get('motif_k')!r}"
    trim = parse_trim(_get(inp, "motif_trim"))
    if trim is None or max(trim) > nat.CDR3_MOTIF_MAX_TRIM:
        return f"--motif-trim is N,C with 0 to {nat.CDR3_MOTIF_MAX_TRIM} each, not {inp.get('motif_trim')!r}"
    min_count = _get(inp, "motif_min_count")
    if not _is_int(min_count) or not 1 <= min_count < 1 << 32:
        return f"--motif-min-count is 1 or more, not {min_count!r}"
    resamples = _get(inp, "resamples")
    if not _is_int(resamples) or not 0 <= resamples <= nat.CDR3_MOTIF_MAX_RESAMPLES:
        return f"--resamples is 0 to {nat.CDR3_MOTIF_MAX_RESAMPLES}, not {resamples!r}"
    seed = _get(inp, "seed")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        return f"--seed is 0 .. 2^64 - 1, not {seed!r}"
    if not inp.get("groups"):
        for flag, key in GROUP_FLAGS:
            if inp.get(key) is not None and inp.get(key) is not False:
                return f"{flag} belongs to --groups: it is refused without it"
        return None
    if resamples == 0:
        return "--groups selects motifs by their p_value: it is refused with --resamples 0"
    p = parse_decimal(_get(inp, "group_p_value"))
    if p is None or not 0 < p <= 1:
        return f"--group-p-value is a decimal above 0 and at most 1, not {inp.get('group_p_value')!r}"
    if parse_decimal(_get(inp, "group_min_fold")) is None:
        return f"--group-min-fold is a decimal, 0 or more, not {inp.get('group_min_fold')!r}"
    distance = _get(inp, "group_distance")
    if not _is_int(distance) or distance not in (0, 1, 2):
        return f"--group-distance is 0, 1 or 2, not {distance!r}"
    return None


def units_of(strings) -> list:
    """The distinct strings in order of first appearance."""
    return list(dict.fromkeys(strings))


def census(units) -> dict:
    """How many units take part, and how many are left out for their length or for a byte outside A..Z."""
    reach = [u for u in units if 1 <= len(u) <= nat.CDR3NET_MAX_LEN]
    take = sum(letters_only(u) for u in reach)
    return {"units": len(units), "take_part": take, "out_of_reach": len(units) - len(reach), "not_letters": len(reach) - take}


def motifs_text(result: dict, resamples: int) -> bytes:
    """The `.cdr3_motifs.tsv` text of one sample's result."""
    R = int(resamples)
    rows = [(int(ge), -int(cs), int(k), nat.cdr3_motif_text(int(k), int(code)), int(cb), int(total), int(mx))
            for k, code, cs, cb, ge, total, mx in zip(*(result[name] for name, _ in nat.CDR3_MOTIF_OUTPUTS))]
    out = ["\t".join(nat.CDR3_MOTIF_COLUMNS)]
    for ge, neg_cs, k, motif, cb, total, mx in sorted(rows):
        cs = -neg_cs
        out.append("\t".join([motif, str(k), str(cs), str(cb), str(R), str(ge), str(total), str(mx), index_fraction(total, R),
                              index_fraction(cs * R, total), index_fraction(ge + 1, R + 1)]))
    return ("\n".join(out) + "\n").encode("ascii")


def selected_rows(result: dict, resamples: int, p: Fraction, fold: Fraction) -> list:
    """The rows of a cdr3_motifs result (motif order) that --groups selects: p_value at most p and fold at least `fold`, in exact
    integer arithmetic — (ge + 1) / (R + 1) <= p, and cs R >= fold sum (so a zero sum passes)."""
    R = int(resamples)
    return [r for r, (cs, ge, total) in enumerate(zip(result["cs"], result["ge"], result["sum"]))
            if (int(ge) + 1) * p.denominator <= p.numerator * (R + 1) and int(cs) * R * fold.denominator >= fold.numerator * int(total)]


def groups_text(units, rows_of, reads_of, selected, groups: dict) -> bytes:
    """The `.cdr3_groups.tsv` text: one line per unit, in unit order."""
    off, mem = groups["mem_off"], groups["mem"]
    held = [[] for _ in units]
    for s, (k, code) in enumerate(selected):
        for i in mem[int(off[s]):int(off[s + 1])]:
            held[int(i)].append(nat.cdr3_motif_text(k, code))
    out = ["\t".join(nat.CDR3_GROUP_COLUMNS)]
    for i, u in enumerate(units):
        g = int(groups["group_of"][i])
        out.append("\t".join([u.decode("latin-1"), str(rows_of[i]), str(reads_of[i]), str(g), str(int(groups["units"][g])),
                              str(int(groups["weight"][g])), str(int(groups["degree"][i])), ",".join(held[i]) or "."]))
    return ("\n".join(out) + "\n").encode("latin-1")


def members_text(units, selected, trim, groups: dict) -> bytes:
    """The `.cdr3_motif_members.tsv` text: lines in (motif order, unit order)."""
    off, mem = groups["mem_off"], groups["mem"]
    out = ["\t".join(nat.CDR3_MOTIF_MEMBER_COLUMNS)]
    for s, (k, code) in enumerate(selected):
        motif = nat.cdr3_motif_text(k, code)
        for i in mem[int(off[s]):int(off[s + 1])]:
            u = units[int(i)]
            at = u.find(motif.encode("ascii"), trim[0], len(u) - trim[1])      # the first window that holds it
            out.append("\t".join([motif, str(k), u.decode("latin-1"), str(at), str(int(groups["group_of"][int(i)]))]))
    return ("\n".join(out) + "\n").encode("latin-1")


def run_groups(inp: dict, name: str, table, s_units, s_off, s_text, result: dict, ks, trim, resamples: int) -> dict:
    """--groups for one sample: the selection from its motifs result, the one call, the printed line and the files."""
    from .io import write_out_motifs
    p_text, fold_text = str(_get(inp, "group_p_value")).strip(), str(_get(inp, "group_min_fold")).strip()
    distance = int(_get(inp, "group_distance"))
    rows = selected_rows(result, resamples, parse_decimal(p_text), parse_decimal(fold_text))
    selected = [(int(result["k"][r]), int(result["code"][r])) for r in rows]
    index = {u: i for i, u in enumerate(s_units)}
    rows_of, reads_of = [0] * len(s_units), [0] * len(s_units)
    for aa, count in zip(table[2], table[3]):
        rows_of[index[aa]] += 1
        reads_of[index[aa]] += count
    groups = nat.cdr3_motif_groups(s_off, s_text, np.array([r % (1 << 64) for r in reads_of], np.uint64), ks, trim, [k for k, _ in selected],
                                   [c for _, c in selected], distance)
    st = groups["stats"]
    print(f"Groups of {name} (motifs with p_value <= {p_text} and fold >= {fold_text}, distance {distance}): {st['units']:,} CDR3s, "
          f"{st['take_part']:,} take part; {st['selected']:,} motifs selected, {st['member_pairs']:,} motif members; "
          f"{st['global_edges']:,} links by distance; {st['groups']:,} groups ({st['singleton_groups']:,} of one CDR3, the largest of "
          f"{st['largest_group']:,}, {st['mixed_groups']:,} with both kinds of link)")
    files = {"groups": write_out_motifs(groups_text(s_units, rows_of, reads_of, selected, groups), name + ".cdr3_groups.tsv", inp)}
    if inp.get("write_motif_members"):
        files["members"] = write_out_motifs(members_text(s_units, selected, trim, groups), name + ".cdr3_motif_members.tsv", inp)
    return {"files": files, "result": groups, "selected": selected, "stats": st}


def run(inp: dict) -> dict:
    """The stage: refusals, the background's units, then per sample its units, the one call, the printed line and the file.
    Returns {"motifs": [names], "results": [...], "stats": [...]}, and with --groups "groups": [run_groups' dicts].  ValueError for what refusal() and read_database() name, for a
    file that is no clonotype table, and for a sample with more units that take part than the background has (both numbers
    named), before the device is touched."""
    from .io import write_out_motifs
    why = refusal(inp)
    if why:
        raise ValueError(why)
    files = list(inp["infile"])
    names = [sample_name(f) for f in files]
    ks, trim = parse_ks(_get(inp, "motif_k")), parse_trim(_get(inp, "motif_trim"))
    min_count, resamples, seed = (int(_get(inp, key)) for key in ("motif_min_count", "resamples", "seed"))
    try:
        db = read_database(inp["background"], {"cdr3_class": "none", "db_cdr3_column": inp.get("bg_cdr3_column") or "junction_aa"})
    except ValueError as e:      # (the column's flag has another name here)
        raise ValueError(str(e).replace("--db-cdr3-column", "--bg-cdr3-column")) from None
    b_units = units_of(db["cdr3"])
    b_census = census(b_units)
    b_off, b_text = spans(b_units)
    out = {"motifs": [], "results": [], "stats": []}
    stats.clear()
    for name, path in zip(names, files):
        table = read_table(path)
        s_units = units_of(table[2])
        s_census = census(s_units)
        if resamples and s_census["take_part"] > b_census["take_part"]:
            raise ValueError(f"{path}: {s_census['take_part']:,} CDR3s take part and the background ({inp['background']}) has only "
                             f"{b_census['take_part']:,} that do: a resample of the sample's size cannot be drawn from it")
        s_off, s_text = spans(s_units)
        result = nat.cdr3_motifs(s_off, s_text, b_off, b_text, ks, trim, min_count, resamples, seed)
        st = result["stats"]
        stats[name] = st
        print(f"Motifs of {name} against {st['background_units']:,} background CDR3s (k {','.join(map(str, ks))}, trim {trim[0]},{trim[1]}, "
              f"at least {min_count}): {st['sample_units']:,} CDR3s, {st['sample_take_part']:,} take part "
              f"({st['sample_out_of_reach']:,} out of reach, {st['sample_not_letters']:,} left out for a byte outside A..Z); "
              f"{st['background_take_part']:,} background CDR3s take part ({st['background_out_of_reach']:,} out of reach, "
              f"{st['background_not_letters']:,} left out for a byte outside A..Z); {st['motifs']:,} distinct motifs, "
              f"{st['reported']:,} reported; {resamples:,} resamples, seed {seed}")
        out["motifs"].append(write_out_motifs(motifs_text(result, resamples), name + ".cdr3_motifs.tsv", inp))
        out["results"].append(result)
        out["stats"].append(st)
        if inp.get("groups"):
            out.setdefault("groups", []).append(run_groups(inp, name, table, s_units, s_off, s_text, result, ks, trim, resamples))
    return out
