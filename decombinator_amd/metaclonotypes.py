"""The `metaclonotypes` sub-command: per clonotype of an antigen-enriched sample, the largest radius of the weighted (TCRdist-style)
CDR3 distance within which a background repertoire almost never falls, and how many of the sample's own clonotypes fall inside
it — tcrdist3's meta-clonotype step.

    python -m decombinator_amd metaclonotypes -in A.clonotypes.tsv [B.clonotypes.tsv.gz ...] -bg background.tsv[.gz]
           [-op DIR] [-pf dcr_] [-dz] [--cdr3-radius 48] [--radius-step 2] [--max-background-rate 1e-5]
           [--cdr3-class none|v|vj] [--strip-alleles] [--cdr3-gap-cost 12] [--cdr3-trim 3,2] [--cdr3-cost-matrix FILE]
           [--bg-cdr3-column NAME] [--bg-v-column NAME] [--bg-j-column NAME]
           [--write-radius-profile] [--write-metaclonotype-members]

The samples are 1 to 64 `.clonotypes.tsv` files (overlap.read_table; a sample is named as `overlap` names it).  The background is
read as `match` reads its database (match.read_database: any tab-separated table with a header line, its columns found by name)
and becomes ONE _native.Cdr3Index on the GPU.  Per sample there are two _native.cdr3_profile_weighted calls (include/dcrx.h
"profile, weighted": per query a histogram of its targets' distances over the whole ladder of radii, from one walk): the sample
against the background's index, and the sample against an index over its own table.  The reference has no counterpart; there is
no CPU fallback.

The ladder is r = 0, step, 2 step, .. --cdr3-radius (a multiple of --radius-step; at most 32 rungs).  The distance, the classes
(numbered from the call STRINGS over the background and all samples), the cost and who takes part (1 .. 32 letters A..Z) are
`match --cdr3-metric weighted`'s.  For a clonotype i that takes part, with M the background entries that take part (in any
class) and B_i(r), S_i(r) the background's and the sample's CDR3s of its class within r (prefix sums of its two rows):
radius_i is the largest r of the ladder with B_i(r) / M <= --max-background-rate, compared exactly as integers
(B_i(r) * denominator <= numerator * M; the rate is read as a fraction from the flag's own text); there is none when r = 0
already fails.  sample_neighbours = S_i(radius_i) - 1: the clonotype meets itself at distance 0 in its own index.
Radius 48, step 2, rate 1e-5 and class v follow tcrdist3's usage: design choices, not measured optima.

Per sample `<prefix><sample>.cdr3_metaclonotypes.tsv[.gz]`: one line per clonotype that takes part, in table order: clonotype (the
0-based row), v_call, j_call, junction_aa, duplicate_count, radius, background_neighbours (B_i at that radius), background (M),
sample_neighbours; `.` in the three computed columns where there is no radius.  --write-radius-profile adds
`<sample>.cdr3_radius_profile.tsv[.gz]`: clonotype, bg_le_<r> for every r of the ladder, then s_le_<r> (cumulative; the sample's
include the clonotype itself).  --write-metaclonotype-members adds `<sample>.cdr3_metaclonotype_members.tsv[.gz]`: clonotype,
radius, member, member_junction_aa, member_duplicate_count, distance — one line per OTHER clonotype of the sample within radius_i
of i, by (clonotype, member), from one _native.cdr3_match_weighted of the sample against its own index at the sample's largest
radius_i, filtered by distance <= radius_i."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _native as nat
from .match import CLASSES, class_key, letters_only, read_database, spans, weighted_refusal, weighted_settings
from .overlap import read_table, sample_name

MAX_SAMPLES = nat.CDR3_MATCH_MAX_SAMPLES
DEFAULTS = {"cdr3_radius": 48, "radius_step": 2, "max_background_rate": "1e-5"}      # after tcrdist3's usage: design choices
COLUMNS = ["clonotype", "v_call", "j_call", "junction_aa", "duplicate_count", "radius", "background_neighbours", "background",
           "sample_neighbours"]
MEMBER_COLUMNS = ["clonotype", "radius", "member", "member_junction_aa", "member_duplicate_count", "distance"]
BG_COLUMNS = {"bg_cdr3_column": "db_cdr3_column", "bg_v_column": "db_v_column", "bg_j_column": "db_j_column"}

stats: dict = {}      # per sample name, the statistics of the last run()


def _get(inp: dict, key: str):
    return inp.get(key) if inp.get(key) is not None else DEFAULTS[key]


def parse_rate(text):
    """--max-background-rate as an exact Fraction of its own text ("1e-5", "0.00001", "1/100000"), or None for what is no number
    or lies outside 0 .. 1."""
    if isinstance(text, bool) or isinstance(text, float):
        text = repr(text)
    try:
        rate = Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError):
        return None
    return rate if 0 <= rate <= 1 else None


def ladder(inp: dict):
    """(step, bins) of arguments refusal() let pass."""
    step = int(_get(inp, "radius_step"))
    return step, int(_get(inp, "cdr3_radius")) // step + 1


def weighted_inp(inp: dict) -> dict:
    """The arguments as match's weighted routines read them: the metric is the weighted one, the radius the ladder's top."""
    return dict(inp, cdr3_metric="weighted", cdr3_distance=1, cdr3_radius=_get(inp, "cdr3_radius"))


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    files = list(inp.get("infile") or [])
    if not 1 <= len(files) <= MAX_SAMPLES:
        return f"metaclonotypes takes 1 to {MAX_SAMPLES} .clonotypes.tsv files (-in), not {len(files)}"
    names = [sample_name(f) for f in files]
    for k, name in enumerate(names):
        if name in names[:k]:
            return f"two files give one sample name ({name!r}): {files[names.index(name)]} and {files[k]}"
    if not inp.get("background"):
        return "metaclonotypes takes a background (-bg): a tab-separated table with a header line"
    step = _get(inp, "radius_step")
    if isinstance(step, bool) or not isinstance(step, int) or not 1 <= step <= nat.CDR3_MAX_RADIUS:
        return f"--radius-step is 1 to {nat.CDR3_MAX_RADIUS}, not {step!r}"
    why = weighted_refusal(weighted_inp(inp))
    if why:
        return why
    radius = _get(inp, "cdr3_radius")
    if radius % step:
        return f"--cdr3-radius is a multiple of --radius-step ({step}), not {radius}"
    if radius // step + 1 > nat.CDR3_PROFILE_MAX_BINS:
        return (f"the ladder 0, {step}, .. {radius} has {radius // step + 1} radii, more than {nat.CDR3_PROFILE_MAX_BINS}: "
                "take a larger --radius-step or a smaller --cdr3-radius")
    if parse_rate(_get(inp, "max_background_rate")) is None:
        return f"--max-background-rate is a decimal or a fraction, 0 to 1, not {_get(inp, 'max_background_rate')!r}"
    if inp.get("cdr3_class", "v") not in CLASSES:
        return f"--cdr3-class is none, v or vj, not {inp['cdr3_class']}"
    return None


def takes_part(s: bytes) -> bool:
    return 1 <= len(s) <= nat.CDR3NET_MAX_LEN and letters_only(s)


def radius_bins(b_cum, M: int, rate: Fraction) -> np.ndarray:
    """Per row of cumulative background counts (rows x bins, ascending along a row) the LAST bin b with
    b_cum[b] * rate.denominator <= rate.numerator * M, or -1 when bin 0 already fails.  The counts are integers, so the test is
    b_cum[b] <= floor(numerator * M / denominator), taken in exact arithmetic."""
    b_cum = np.asarray(b_cum, dtype=np.uint64)
    most = (rate.numerator * int(M)) // rate.denominator
    passes = b_cum <= np.uint64(min(most, (1 << 64) - 1))
    return passes.sum(axis=1).astype(np.int64) - 1      # (monotone rows: the passing bins are a prefix)


def read_background(inp: dict) -> dict:
    """The background through match.read_database, with the --bg-* columns in the --db-* columns' place."""
    as_db = {"cdr3_class": inp.get("cdr3_class", "v")}
    for bg, db in BG_COLUMNS.items():
        as_db[db] = inp.get(bg)
    try:
        return read_database(inp["background"], as_db)
    except ValueError as e:
        raise ValueError(str(e).replace("--db-", "--bg-")) from None


def table_text(rows, v, j, aa, dup, r_bin, b_cum, s_cum, M: int, step: int) -> bytes:
    out = ["\t".join(COLUMNS).encode()]
    for i in rows:
        head = [str(i).encode(), v[i].encode("latin-1"), j[i].encode("latin-1"), aa[i], str(dup[i]).encode()]
        b = int(r_bin[i])
        tail = [b"."] * 2 + [str(M).encode(), b"."] if b < 0 else [
            str(b * step).encode(), str(int(b_cum[i, b])).encode(), str(M).encode(), str(int(s_cum[i, b]) - 1).encode()]
        out.append(b"\t".join(head + tail))
    return b"\n".join(out) + b"\n"


def profile_text(rows, b_cum, s_cum, step: int, bins: int) -> bytes:
    head = ["clonotype"] + [f"bg_le_{b * step}" for b in range(bins)] + [f"s_le_{b * step}" for b in range(bins)]
    out = ["\t".join(head).encode()]
    for i in rows:
        out.append("\t".join([str(i)] + [str(int(x)) for x in b_cum[i]] + [str(int(x)) for x in s_cum[i]]).encode())
    return b"\n".join(out) + b"\n"


def members_text(index, classes, off, text, aa, dup, cost, r_bin, step: int) -> bytes:
    """One cdr3_match_weighted of the sample against its own index at the largest radius of the sample; the hits within each
    clonotype's own radius, without the clonotype itself (rows are by clonotype, and a row's targets ascend)."""
    out = ["\t".join(MEMBER_COLUMNS).encode()]
    if len(r_bin) and int(r_bin.max()) >= 0:
        result = nat.cdr3_match_weighted(index, classes, off, text, np.ones(len(aa), dtype=np.uint64), cost, int(r_bin.max()) * step)
        hit, dist = np.asarray(result["hit"], dtype=np.int64), np.asarray(result["hit_dist"], dtype=np.int64)
        owner = np.repeat(np.arange(len(aa), dtype=np.int64), np.diff(np.asarray(result["hit_off"], dtype=np.int64)))
        keep = (dist <= r_bin[owner] * step) & (hit != owner)
        for i, m, d in zip(owner[keep].tolist(), hit[keep].tolist(), dist[keep].tolist()):
            out.append(b"\t".join([str(i).encode(), str(int(r_bin[i]) * step).encode(), str(m).encode(), aa[m], str(dup[m]).encode(),
                                   str(d).encode()]))
    return b"\n".join(out) + b"\n"


def run(inp: dict) -> dict:
    """The stage: refusals, the cost, the background and its index, then per sample the two profiles, the radii, the printed line
    and the files.  Returns {"metaclonotypes": [names], "profiles": [names], "members": [names], "results": [...], "stats":
    [...]}.  ValueError for what refusal() and match.read_database() name and for a file that is no clonotype table."""
    from .io import write_out_metaclonotypes
    why = refusal(inp)
    if why:
        raise ValueError(why)
    files = list(inp["infile"])
    names = [sample_name(f) for f in files]
    mode, strip = inp.get("cdr3_class", "v"), bool(inp.get("strip_alleles"))
    step, bins = ladder(inp)
    rate = parse_rate(_get(inp, "max_background_rate"))
    cost, radius = weighted_settings(weighted_inp(inp))      # (the matrix file: before the background)
    bg = read_background(inp)
    class_no = {}
    t_classes = [class_no.setdefault(class_key(mode, v, j, strip), len(class_no)) for v, j in zip(bg["v"], bg["j"])]
    t_off, t_text = spans(bg["cdr3"])
    M = sum(takes_part(s) for s in bg["cdr3"])
    out = {"metaclonotypes": [], "profiles": [], "members": [], "results": [], "stats": []}
    stats.clear()
    index = nat.Cdr3Index(np.array(t_classes, dtype=np.uint32), t_off, t_text)
    try:
        for name, path in zip(names, files):
            v, j, aa, dup = read_table(path)
            classes = np.array([class_no.setdefault(class_key(mode, a, b, strip), len(class_no)) for a, b in zip(v, j)], dtype=np.uint32)
            off, text = spans(aa)
            against_bg = nat.cdr3_profile_weighted(index, classes, off, text, cost, step, bins)
            own = nat.Cdr3Index(classes, off, text)
            try:
                against_own = nat.cdr3_profile_weighted(own, classes, off, text, cost, step, bins)
                b_cum = np.cumsum(np.asarray(against_bg["profile"], dtype=np.uint64).reshape(len(aa), bins), axis=1, dtype=np.uint64)
                s_cum = np.cumsum(np.asarray(against_own["profile"], dtype=np.uint64).reshape(len(aa), bins), axis=1, dtype=np.uint64)
                rows = [i for i, s in enumerate(aa) if takes_part(s)]
                r_bin = np.full(len(aa), -1, dtype=np.int64)
                if rows:
                    r_bin[rows] = radius_bins(b_cum[rows], M, rate)
                members = (members_text(own, classes, off, text, aa, dup, cost, r_bin, step)
                           if inp.get("write_metaclonotype_members") else None)
            finally:
                own.close()
            with_radius = [i for i in rows if r_bin[i] >= 0]
            st = {"clonotypes": len(aa), "take_part": len(rows), "not_letters": against_bg["stats"]["queries_not_letters"],
                  "out_of_reach": against_bg["stats"]["queries_out_of_reach"], "background": len(bg["cdr3"]), "background_take_part": M,
                  "with_radius": len(with_radius),
                  "with_neighbours": sum(int(s_cum[i, r_bin[i]]) > 1 for i in with_radius)}
            stats[name] = st
            print(f"Meta-clonotypes of {name} against {M:,} background CDR3s (radii 0 to {radius} by {step}, at most {rate} of the "
                  f"background, gap {cost.gap}, trim {cost.ntrim},{cost.ctrim}, class {mode}): {st['clonotypes']:,} clonotypes, "
                  f"{st['take_part']:,} take part ({st['not_letters']:,} left out for a byte outside A..Z, {st['out_of_reach']:,} out of "
                  f"reach), {st['with_radius']:,} with a radius, {st['with_neighbours']:,} of them with a sample neighbour")
            out["metaclonotypes"].append(write_out_metaclonotypes(table_text(rows, v, j, aa, dup, r_bin, b_cum, s_cum, M, step),
                                                                  name + ".cdr3_metaclonotypes.tsv", inp))
            if inp.get("write_radius_profile"):
                out["profiles"].append(write_out_metaclonotypes(profile_text(rows, b_cum, s_cum, step, bins),
                                                                name + ".cdr3_radius_profile.tsv", inp))
            if members is not None:
                out["members"].append(write_out_metaclonotypes(members, name + ".cdr3_metaclonotype_members.tsv", inp))
            out["results"].append({"background": against_bg, "sample": against_own, "radius_bin": r_bin})
            out["stats"].append(st)
    finally:
        index.close()
    return out
