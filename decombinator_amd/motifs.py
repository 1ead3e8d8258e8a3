"""The `motifs` sub-command: which short motifs — 2-, 3- and 4-mers in the hypervariable middle of the CDR3 — occur in more of a
sample's CDR3s than in as many CDR3s drawn from a background repertoire (GLIPH's "local" question, beside the "global" one
`match` and `--cdr3-network` answer).

    python -m decombinator_amd motifs -in A.clonotypes.tsv [B.clonotypes.tsv.gz ...] -bg naive.clonotypes.tsv[.gz]
           [--bg-cdr3-column junction_aa] [--motif-k 2,3,4] [--motif-trim 3,3] [--motif-min-count 3]
           [--resamples 1000] [--seed 1] [-op DIR] [-pf dcr_] [-dz]

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
at six decimals, `nan` on a zero denominator."""
from __future__ import annotations

from . import _native as nat
from .match import letters_only, parse_trim, read_database, spans
from .overlap import index_fraction, read_table, sample_name

DEFAULTS = {"motif_k": "2,3,4", "motif_trim": "3,3", "motif_min_count": 3, "resamples": 1000, "seed": 1}      # design choices (3,3 and 3 after GLIPH)

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


def run(inp: dict) -> dict:
    """The stage: refusals, the background's units, then per sample its units, the one call, the printed line and the file.
    Returns {"motifs": [names], "results": [...], "stats": [...]}.  ValueError for what refusal() and read_database() name, for a
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
        s_units = units_of(read_table(path)[2])
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
    return out
