"""The `associate` sub-command: which features of a feature by sample table — the meta-clonotypes of a `tabulate.tsv`, or the
public clonotypes of an `overlap_public.tsv` — are present in the cases of a cohort more (or less) often than in its controls:
an exact test per feature, and a label-permutation null over ALL features at once for the multiple-testing correction (the null
of Emerson et al. 2017 for public CMV clonotypes; what tcrdist3 users run after the bulk tabulation).

    python -m decombinator_amd associate -in out/dcr_tabulate.tsv.gz [more.tsv.gz ...] -ph cohort.tsv --case LABEL [-op DIR]
           [-pf dcr_] [-dz] [--ph-sample-column sample] [--ph-group-column group] [--value clonotypes|reads] [--min-count 1]
           [--alternative greater|less|two-sided] [--permutations 10000] [--seed 1] [--max-p 0.05] [--write-null]
           [--test fisher|rank-sum] [--depths dcr_tabulate_samples.tsv]

-in is a table, plain or .gz, recognised by its header: a tabulate.tsv (first column `metaclonotype`; sample X's value is the
column X_clonotypes, or X_reads under --value reads) or an overlap_public.tsv (sample X's value is the column X: reads, so
--value clonotypes is refused there).  SEVERAL tabulate.tsv — the runs of `tabulate` over one -mc file, 64 samples each — are
joined side by side: their identity columns must hold the same rows in the same order, no sample may occur twice, and the
samples stand in file order, then column order; more than one overlap_public.tsv is refused (a clonotype missing from one run's
file was in fewer than --min-samples of that run's samples, not in none).  -ph is a tab-separated table with a header whose
sample and group columns are found by name; a group of `.` or nothing means unknown (the sample is left out and counted), the
rest hold exactly two labels and --case names one.  A sample of -ph without a column in -in is an error; a sample of -in
without a row in -ph is left out and named in a printed line.  The N samples used (2 .. 1024, at least one per group) stand in
-in's column order.  Up to 64 samples used a presence pattern is one word and _native.assoc_permute runs, every file and line as
it always was; from 65 on patterns are rows of ceil(N / 64) words, de-duplicated by row and handed over in ascending popcount,
the table of ranks is built by cumulative sums (rank_table_sums) and holds 32-bit ranks, and _native.assoc_permute_wide runs
(include/dcrx.h "association, wide").

A feature is PRESENT in a sample when its value is at least --min-count: THE TEST IS ON PRESENCE, NOT ABUNDANCE.  With n1 cases,
n0 controls, a feature present in m samples, k of them cases, and h(x) = C(n1, x) C(n0, m - x), the p-value is, in exact
fractions of Python integers: `greater` (the default, as Emerson's) the sum of h(x) over x >= k, `less` over x <= k, `two-sided`
over the x with h(x) <= h(k), each over C(N, m).  All (m, k) a cohort can produce are a table of (N + 1)^2 cells; its cells are
ranked (dense: equal fractions share a rank), and everything on the device is done on RANKS — integers only, exact.  The
features are de-duplicated by presence pattern on the host (np.unique: a cohort's rare features have few patterns however many
clonotypes carry them), and ONE _native.assoc_permute call (include/dcrx.h "association") scores every pattern under every one of
--permutations relabelings of the samples, drawn from --seed by the counter-based key `overlap --downsample` uses: per
relabeling the smallest rank (perm_min), per rank at or below --max-p the (feature, relabeling) pairs that reach it (tail).
With --permutations 0 no native call is made and the stage needs no GPU.  The reference has no counterpart; with permutations
there is no CPU fallback.  `greater`, 10 000 permutations and 0.05 are design choices after Emerson et al., not measured optima.

Derived, as exact fractions: p_adjusted(f) = (1 + #{p : perm_min[p] <= rank(f)}) / (P + 1), Westfall and Young's single-step
min-P; for a tail rank r, O(r) = the features at ranks <= r, V(r) = the sum of tail[r'] over r' <= r, fdr(r) = min(1, V(r) /
(P O(r))), and q_value(f) = the smallest fdr(r) over r >= rank(f): the permutation FDR, made monotone.

`<prefix>associate.tsv[.gz]`: one line per feature of -in, most significant first (by rank, then by file order): the identity
columns verbatim, present, present_cases, present_controls, cases, controls, odds_ratio, p_value, p_adjusted, q_value (`.`
where the p-value is above --max-p; both `.` without permutations).
`<prefix>associate_null.tsv[.gz]` (--write-null): per tail rank: rank, p_value, features, features_cumulative, null_pairs,
null_cumulative, expected_false (V / P), fdr.

--test rank-sum (include/dcrx.h "association, rank-sum") asks the other question: is a feature's VALUE — its breadth or
depth in a sample — higher (or lower) in the cases, whether or not it is present in more of them.  2 to 64 samples used.  Per
feature the values below --min-count count as 0, the samples are ranked with ties sharing the mid-rank — by value, or by value
over the sample's depth under --depths (a table with a `sample` column and one named as --value: a tabulate_samples.tsv fits),
compared by cross-multiplication in integers — and the Wilcoxon / Mann-Whitney rank sum of the cases is standardized in fixed
point: with doubled mid-ranks d less their minimum, a = d - min d, A = sum a, B = sum a^2, Q = N B - A^2, W the sum of a over
the cases and D = N W - n1 A, the score is t = (u min(2^32 - 1, isqrt(2^64 / Q))) >> 20, u = D, -D or |D| clamped to 20 bits;
z = D sqrt((N - 1) / (n1 n0 Q)) is the usual statistic (no continuity correction), and t is z times one factor for all features.
Rows of equal scores are de-duplicated, and ONE _native.assoc_ranksum call scores every row under every relabeling — the
relabelings of the default test, word for word.  Derived, as exact fractions: p_value = (1 + #{p : t_p(f) >= t(f)}) / (P + 1),
the feature's own permutation p-value; p_adjusted = (1 + #{p : max_f t_p(f) >= t(f)}) / (P + 1), Westfall and Young's
single-step max-T; over the edges e — the up to 1024 largest distinct observed scores — O(e) = the features scoring at least
e, V(e) = the null's pairs scoring at least e, fdr(e) = min(1, V / (P O)) and q_value = the smallest fdr over the edges at or
below the feature's score (`.` below the lowest edge).  --max-p has no role there and is refused; --depths is refused under the
default test.  associate.tsv then holds the identity columns, nonzero, nonzero_cases, nonzero_controls, cases, controls,
mean_rank_cases, mean_rank_controls, z, score, p_value, p_adjusted, q_value, highest score first; associate_null.tsv per edge,
highest first: score, z, features, features_cumulative, null_pairs, null_cumulative, expected_false, fdr."""
from __future__ import annotations

import gzip
from fractions import Fraction
from math import comb, isqrt, sqrt

import numpy as np

from . import _native as nat

MAX_SAMPLES = nat.ASSOC_MAX_SAMPLES                # up to here the narrow entry: a pattern is one word, a rank 16 bits
WIDE_MAX_SAMPLES = nat.ASSOC_WIDE_MAX_SAMPLES      # up to here the wide entry: patterns of up to 16 words, ranks of 32 bits
ANNOUNCE_TABLE_ABOVE = 256                         # samples from which on the table build is announced: it takes seconds
ALTERNATIVES = ("greater", "less", "two-sided")
TESTS = ("fisher", "rank-sum")
VALUES = ("clonotypes", "reads")
DEFAULTS = {"alternative": "greater", "permutations": 10000, "max_p": "0.05", "seed": 1, "min_count": 1,      # after Emerson et
            "ph_sample_column": "sample", "ph_group_column": "group"}                                          # al.: design choices
TABULATE_IDENTITY = ["metaclonotype", "v_call", "j_call", "junction_aa", "radius"]
TABULATE_COLUMNS = TABULATE_IDENTITY + ["samples"]
PUBLIC_IDENTITY = nat.OVERLAP_PUBLIC_COLUMNS[:3]
RESULT_COLUMNS = ["present", "present_cases", "present_controls", "cases", "controls", "odds_ratio", "p_value", "p_adjusted", "q_value"]
NULL_COLUMNS = ["rank", "p_value", "features", "features_cumulative", "null_pairs", "null_cumulative", "expected_false", "fdr"]
RANKSUM_RESULT_COLUMNS = ["nonzero", "nonzero_cases", "nonzero_controls", "cases", "controls", "mean_rank_cases", "mean_rank_controls", "z",
                          "score", "p_value", "p_adjusted", "q_value"]
RANKSUM_NULL_COLUMNS = ["score", "z", "features", "features_cumulative", "null_pairs", "null_cumulative", "expected_false", "fdr"]
NO_RANK = 0xFFFF      # what a cell no cohort can produce holds in the table (never read)
NO_RANK_WIDE = 0xFFFFFFFF      # ... and in the wide layer's table of 32-bit ranks

stats: dict = {}      # the statistics of the last run()


def _get(inp: dict, key: str):
    return inp.get(key) if inp.get(key) is not None else DEFAULTS[key]


def parse_max_p(text):
    """--max-p as an exact Fraction of its own text ("0.05", "5e-2", "1/20"), or None for what is no number or lies outside 0 .. 1."""
    if isinstance(text, (bool, float)):
        text = repr(text)
    try:
        p = Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError):
        return None
    return p if 0 <= p <= 1 else None


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    test = inp.get("test") if inp.get("test") is not None else "fisher"
    if test not in TESTS:
        return f"--test is fisher or rank-sum, not {inp['test']}"
    if test == "rank-sum" and inp.get("max_p") is not None:
        return ("--max-p has no role under --test rank-sum: the tail is the up to 1024 largest distinct observed scores.  Leave it "
                "out")
    if test == "fisher" and inp.get("depths"):
        return "--depths only works with --test rank-sum: the default test is on presence, and a depth does not change presence"
    if not inp.get("infile"):
        return ("associate takes its table (-in): a tabulate.tsv of `tabulate` — or several, the runs over one -mc file — or an "
                "overlap_public.tsv of `overlap`, plain or .gz")
    if not inp.get("phenotype"):
        return "associate takes the cohort (-ph): a tab-separated table with a header line, a sample and a group column"
    if inp.get("case") in (None, "", "."):
        return "associate takes the label of the cases (--case): one of the two labels of the -ph group column"
    if inp.get("value") not in (None,) + VALUES:
        return f"--value is clonotypes or reads, not {inp['value']}"
    if _get(inp, "alternative") not in ALTERNATIVES:
        return f"--alternative is greater, less or two-sided, not {inp['alternative']}"
    if int(_get(inp, "min_count")) < 1:
        return f"--min-count is 1 or more, not {inp['min_count']}"
    if not 0 <= int(_get(inp, "permutations")) <= nat.ASSOC_MAX_PERMUTATIONS:
        return f"--permutations is 0 to {nat.ASSOC_MAX_PERMUTATIONS} (2^20), not {inp['permutations']}"
    if not 0 <= int(_get(inp, "seed")) < 1 << 64:
        return f"--seed is 0 to 2^64 - 1, not {inp['seed']}"
    if parse_max_p(_get(inp, "max_p")) is None:
        return f"--max-p is a decimal or a fraction, 0 to 1, not {_get(inp, 'max_p')!r}"
    return None


# ---- the test: every p-value a cohort of n1 cases among N samples can produce ----

def feasible(N: int, n1: int, m: int) -> range:
    """The k a feature present in m of N samples can have among n1 cases."""
    return range(max(0, m - (N - n1)), min(m, n1) + 1)


def fisher_table(N: int, n1: int, alternative: str) -> dict:
    """{(m, k): the exact p-value as a Fraction} over the feasible cells."""
    n0, out = N - n1, {}
    for m in range(N + 1):
        ks = feasible(N, n1, m)
        h = {x: comb(n1, x) * comb(n0, m - x) for x in ks}
        total = comb(N, m)
        for k in ks:
            if alternative == "greater":
                num = sum(h[x] for x in ks if x >= k)
            elif alternative == "less":
                num = sum(h[x] for x in ks if x <= k)
            else:
                num = sum(h[x] for x in ks if h[x] <= h[k])
            out[(m, k)] = Fraction(num, total)
    return out


def rank_table(N: int, n1: int, alternative: str):
    """(table, p_of_rank): the (N + 1) x (N + 1) uint16 table of dense ranks of the p-values, smaller = more extreme (NO_RANK
    where a cell is not feasible), and the p-value of every rank, ascending."""
    cells = fisher_table(N, n1, alternative)
    p_of_rank = sorted(set(cells.values()))
    rank_of = {p: r for r, p in enumerate(p_of_rank)}
    table = np.full((N + 1, N + 1), NO_RANK, dtype=np.uint16)
    for (m, k), p in cells.items():
        table[m, k] = rank_of[p]
    return table, p_of_rank


def rank_table_sums(N: int, n1: int, alternative: str):
    """rank_table() for cohorts of any size — the same Fractions and the same dense ranks, as an (N + 1) x (N + 1) uint32 table
    (NO_RANK_WIDE where a cell is not feasible) — by cumulative sums: fisher_table() sums a row's h(x) again for every k and is
    cubic in N; here a row is one pass from the top (greater) or from the bottom (less), and for two-sided one sort of the
    row's h(x), equal h sharing the sum up to the end of their group.  A balanced cohort of 1024 has 131 074 ranks under
    `greater`; the build takes seconds on one CPU thread (profiles/assoc_wide/bench_assoc_wide.json, "tables", has the times of
    the recorded run)."""
    n0 = N - n1
    of_cases, of_controls = [comb(n1, x) for x in range(n1 + 1)], [comb(n0, y) for y in range(n0 + 1)]
    cells = {}
    for m in range(N + 1):
        ks = feasible(N, n1, m)
        h = [of_cases[x] * of_controls[m - x] for x in ks]
        num, run = [0] * len(h), 0
        if alternative == "greater":
            for i in range(len(h) - 1, -1, -1):
                run += h[i]
                num[i] = run
        elif alternative == "less":
            for i in range(len(h)):
                run += h[i]
                num[i] = run
        else:
            order = sorted(range(len(h)), key=h.__getitem__)
            a = 0
            while a < len(order):
                b = a
                while b < len(order) and h[order[b]] == h[order[a]]:
                    run += h[order[b]]
                    b += 1
                for i in order[a:b]:
                    num[i] = run
                a = b
        total = comb(N, m)
        for k, x in zip(ks, num):
            cells[(m, k)] = Fraction(x, total)
    p_of_rank = sorted(set(cells.values()))
    rank_of = {p: r for r, p in enumerate(p_of_rank)}
    table = np.full((N + 1, N + 1), NO_RANK_WIDE, dtype=np.uint32)
    for (m, k), p in cells.items():
        table[m, k] = rank_of[p]
    return table, p_of_rank


# ---- the two files ----

def _lines(path: str):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [x[:-1] if x.endswith(b"\r") else x for x in lines]


def read_features(path: str, value):
    """-in: {"kind": "tabulate" or "public", "identity": the identity columns' names, "rows": per feature its identity cells
    joined by tabs (bytes, verbatim), "samples": the sample names in column order, "values": features x samples (int64),
    "value": what the values are}.  ValueError for a header that is neither table's (naming it), --value clonotypes on an
    overlap_public.tsv, a short line and a value that is no integer, by line."""
    lines = _lines(path)
    header = [h.decode("utf-8", "replace") for h in lines[0].split(b"\t")] if lines else []
    if header[:len(TABULATE_COLUMNS)] == TABULATE_COLUMNS:
        kind, identity, value = "tabulate", TABULATE_IDENTITY, value or "clonotypes"
        rest = header[len(TABULATE_COLUMNS):]
        suffix = "_" + value
        at = {h[:-len(suffix)]: len(TABULATE_COLUMNS) + i for i, h in enumerate(rest) if h.endswith(suffix)}
        samples = [h[:-len("_clonotypes")] for h in rest if h.endswith("_clonotypes")]
        if len(rest) != 2 * len(samples) or any(s not in at for s in samples):
            raise ValueError(f"{path}: a tabulate.tsv holds <sample>_clonotypes and <sample>_reads per sample; its header is " + "\t".join(header))
    elif header[:len(nat.OVERLAP_PUBLIC_COLUMNS)] == nat.OVERLAP_PUBLIC_COLUMNS:
        if value == "clonotypes":
            raise ValueError(f"{path} is an overlap_public.tsv: it holds reads per sample, so --value clonotypes cannot be served")
        kind, identity, value = "public", PUBLIC_IDENTITY, "reads"
        samples = header[len(nat.OVERLAP_PUBLIC_COLUMNS):]
        at = {s: len(nat.OVERLAP_PUBLIC_COLUMNS) + i for i, s in enumerate(samples)}
    else:
        raise ValueError(f"{path} is neither a tabulate.tsv (first columns {', '.join(TABULATE_COLUMNS)}) nor an overlap_public.tsv "
                         f"(first columns {', '.join(nat.OVERLAP_PUBLIC_COLUMNS)}); its header is {' '.join(header)!r}")
    for k, s in enumerate(samples):
        if s in samples[:k]:
            raise ValueError(f"{path}: the sample {s!r} has two columns")
    where_id = [header.index(c) for c in identity]
    where = [at[s] for s in samples]
    rows, values = [], np.zeros((len(lines) - 1, len(samples)), dtype=np.int64)
    for n, line in enumerate(lines[1:], 2):
        f = line.split(b"\t")
        if len(f) < len(header):
            raise ValueError(f"{path}, line {n}: {len(f)} fields, fewer than the header's {len(header)}")
        rows.append(b"\t".join(f[i] for i in where_id))
        for c, i in enumerate(where):
            if not f[i].isdigit():
                raise ValueError(f"{path}, line {n}: the value {f[i].decode('latin-1')!r} of sample {samples[c]!r} is no count")
            values[n - 2, c] = int(f[i])
    return {"kind": kind, "identity": identity, "rows": rows, "samples": samples, "values": values, "value": value}


def infiles(inp: dict) -> list:
    """-in as a list of paths: run() takes one path or a list of them."""
    given = inp.get("infile")
    return [given] if isinstance(given, (str, bytes)) or hasattr(given, "__fspath__") else list(given or [])


def join_features(paths: list, value):
    """-in of several tables: the runs of `tabulate` over ONE -mc file, 64 samples each, side by side.  Every file is a
    tabulate.tsv whose identity columns hold the same rows in the same order; the joined samples stand in file order, then
    column order.  ValueError for an overlap_public.tsv among several (a clonotype missing from one run's file was in fewer
    than --min-samples of THAT run's samples, not in none of them: the files cannot be joined), for rows that differ (naming the
    first file and line that do) and for a sample that occurs in two files."""
    tables = [read_features(p, value) for p in paths]
    first = tables[0]
    if len(tables) == 1:
        return first
    for p, t in zip(paths, tables):
        if t["kind"] != "tabulate":
            raise ValueError(f"{p} is an overlap_public.tsv, and -in holds {len(paths)} tables: only the tabulate.tsv runs over one -mc file "
                             "can be joined.  A clonotype missing from one run's overlap_public.tsv was in fewer than --min-samples of "
                             "that run's samples, not in none of them")
    seen = {s: paths[0] for s in first["samples"]}
    for p, t in zip(paths[1:], tables[1:]):
        for n, (a, b) in enumerate(zip(first["rows"], t["rows"]), 2):
            if a != b:
                raise ValueError(f"{p}, line {n}: its identity columns ({', '.join(TABULATE_IDENTITY)}) are not those of {paths[0]}, line "
                                 f"{n}: the tables of -in are runs of `tabulate` over one -mc file")
        if len(t["rows"]) != len(first["rows"]):
            n = min(len(t["rows"]), len(first["rows"])) + 2
            raise ValueError(f"{p}, line {n}: {p} holds {len(t['rows'])} meta-clonotypes and {paths[0]} holds {len(first['rows'])}: the tables "
                             "of -in are runs of `tabulate` over one -mc file")
        for s in t["samples"]:
            if s in seen:
                raise ValueError(f"the sample {s!r} has a column in {seen[s]} and in {p}")
            seen[s] = p
    return {"kind": "tabulate", "identity": first["identity"], "rows": first["rows"], "samples": [s for t in tables for s in t["samples"]],
            "values": np.concatenate([t["values"] for t in tables], axis=1), "value": first["value"]}


def read_phenotype(path: str, sample_column: str, group_column: str) -> dict:
    """-ph: {sample: group} in file order, the group "" for unknown (`.` or nothing).  ValueError for a missing column (naming
    the file's), a short line and a sample with two rows."""
    lines = _lines(path)
    if not lines:
        raise ValueError(f"{path} has no header line")
    header = [h.decode("utf-8", "replace") for h in lines[0].split(b"\t")]
    for name, flag in ((sample_column, "--ph-sample-column"), (group_column, "--ph-group-column")):
        if name not in header:
            raise ValueError(f"{path} has no column {name!r} ({flag}); its columns are " + ", ".join(header))
    at_s, at_g = header.index(sample_column), header.index(group_column)
    out = {}
    for n, line in enumerate(lines[1:], 2):
        f = [x.decode("utf-8", "replace") for x in line.split(b"\t")]
        if len(f) <= max(at_s, at_g):
            raise ValueError(f"{path}, line {n}: {len(f)} fields, fewer than the header's {len(header)}")
        if f[at_s] in out:
            raise ValueError(f"{path}, line {n}: the sample {f[at_s]!r} has two rows")
        group = f[at_g].strip()
        out[f[at_s]] = "" if group == "." else group
    return out


def cohort(features: dict, groups: dict, case: str, path_in: str, path_ph: str) -> dict:
    """Who takes part: {"used": column indices of -in in column order, "names", "case_mask" (bit i: used sample i is a case),
    "n1", "n0", "unknown": samples of -ph without a group, "not_in_ph": samples of -in without a row}."""
    have = set(features["samples"])
    for s in groups:
        if s not in have:
            raise ValueError(f"{path_ph}: the sample {s!r} has no column in {path_in}")
    labels = sorted({g for g in groups.values() if g})
    if len(labels) != 2:
        raise ValueError(f"{path_ph}: the group column holds {len(labels)} labels ({', '.join(labels) or 'none'}), not two")
    if case not in labels:
        raise ValueError(f"--case {case!r} is none of the two labels of {path_ph}: {labels[0]!r}, {labels[1]!r}")
    used = [i for i, s in enumerate(features["samples"]) if groups.get(s)]
    names = [features["samples"][i] for i in used]
    case_mask = sum(1 << b for b, s in enumerate(names) if groups[s] == case)
    n1 = bin(case_mask).count("1")
    if not 2 <= len(used) <= WIDE_MAX_SAMPLES:
        raise ValueError(f"associate takes 2 to {WIDE_MAX_SAMPLES} samples with a group, not {len(used)}")
    if n1 == 0 or n1 == len(used):
        raise ValueError(f"every one of the {len(used)} samples used is a {'case' if n1 else 'control'}: at least one sample per group")
    return {"used": used, "names": names, "case_mask": case_mask, "n1": n1, "n0": len(used) - n1,
            "unknown": [s for s, g in groups.items() if not g], "not_in_ph": [s for s in features["samples"] if s not in groups]}


def presence_masks(values: np.ndarray, used, min_count: int) -> np.ndarray:
    masks = np.zeros(values.shape[0], dtype=np.uint64)
    for b, i in enumerate(used):
        masks |= (values[:, i] >= min_count).astype(np.uint64) << np.uint64(b)
    return masks


def presence_words(values: np.ndarray, used, min_count: int) -> np.ndarray:
    """The presence patterns of a cohort of any size: features x ceil(N / 64) words, used sample b at bit b & 63 of word b >> 6."""
    words = np.zeros((values.shape[0], (len(used) + 63) // 64), dtype=np.uint64)
    for b, i in enumerate(used):
        words[:, b >> 6] |= (values[:, i] >= min_count).astype(np.uint64) << np.uint64(b & 63)
    return words


def popcount_rows(words: np.ndarray) -> np.ndarray:
    """Per row of a features x words array the bits set (int64)."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(words).astype(np.int64).sum(axis=1)
    return np.unpackbits(words.view(np.uint8), axis=1).astype(np.int64).sum(axis=1)


def case_words(case_mask: int, N: int) -> np.ndarray:
    return np.array([(case_mask >> (64 * w)) & ((1 << 64) - 1) for w in range((N + 63) // 64)], dtype=np.uint64)


# ---- --test rank-sum: scores on the host, in integers ----

def read_depths(path: str, value: str) -> dict:
    """--depths: {sample: depth} from a tab-separated table with a `sample` column and one named as --value (a
    tabulate_samples.tsv fits as it stands).  ValueError for a missing column, a short line, a depth that is no count and a
    sample with two rows."""
    lines = _lines(path)
    if not lines:
        raise ValueError(f"{path} has no header line")
    header = [h.decode("utf-8", "replace") for h in lines[0].split(b"\t")]
    for name in ("sample", value):
        if name not in header:
            raise ValueError(f"{path} (--depths) has no column {name!r}; its columns are " + ", ".join(header))
    at_s, at_v = header.index("sample"), header.index(value)
    out = {}
    for n, line in enumerate(lines[1:], 2):
        f = line.split(b"\t")
        if len(f) <= max(at_s, at_v):
            raise ValueError(f"{path}, line {n}: {len(f)} fields, fewer than the header's {len(header)}")
        name = f[at_s].decode("utf-8", "replace")
        if name in out:
            raise ValueError(f"{path}, line {n}: the sample {name!r} has two rows")
        if not f[at_v].isdigit():
            raise ValueError(f"{path}, line {n}: the depth {f[at_v].decode('latin-1')!r} of sample {name!r} is no count")
        out[name] = int(f[at_v])
    return out


def rank_scores(values: np.ndarray, used, min_count: int, depths=None, names=None) -> np.ndarray:
    """The a-matrix of the rank-sum test, features x len(used) (int64): per feature x[s] = the value of used sample s, 0 where it
    is below min_count; d[s] = 2 #{t : x[t] < x[s]} + #{t : x[t] = x[s]} + 1, the doubled mid-rank; a[s] = d[s] - min d, so the
    samples holding the smallest value score 0 and a <= 2 N - 2.  depths (one int per used sample, or None): the samples are
    ordered by x[s] / depths[s] instead, compared by cross-multiplication in integers; ValueError for a depth of 0 under a
    non-zero value, naming the sample (names[s], or its number)."""
    x = np.asarray(values, dtype=np.int64)[:, list(used)]
    x = np.where(x >= min_count, x, 0)
    F, N = x.shape
    if depths is not None:
        depths = [int(v) for v in depths]
        if len(depths) != N:
            raise ValueError(f"rank_scores: {len(depths)} depths for {N} samples")
        for s in range(N):
            if depths[s] == 0 and F and int(x[:, s].max()) > 0:
                raise ValueError(f"--depths: the sample {names[s] if names else s!r} has a depth of 0 and a non-zero value")
        a = np.zeros((F, N), dtype=np.int64)
        for f in np.flatnonzero(x.any(axis=1)):      # (a row of zeros scores 0 everywhere)
            key = [Fraction(int(v), d) if v else Fraction(0) for v, d in zip(x[f], depths)]      # Fractions compare by cross-multiplication
            d2 = [2 * sum(k < mine for k in key) + sum(k == mine for k in key) + 1 for mine in key]
            a[f] = np.array(d2, dtype=np.int64) - min(d2)
        return a
    if not F:
        return np.zeros((0, N), dtype=np.int64)
    order = np.argsort(x, axis=1, kind="stable")
    ranked = np.take_along_axis(x, order, axis=1)
    at = np.broadcast_to(np.arange(N, dtype=np.int64), (F, N))
    fresh = np.ones((F, N), dtype=bool)
    fresh[:, 1:] = ranked[:, 1:] != ranked[:, :-1]
    first = np.maximum.accumulate(np.where(fresh, at, 0), axis=1)      # where the run of equal values begins: the values below
    last_flag = np.ones((F, N), dtype=bool)
    last_flag[:, :-1] = fresh[:, 1:]
    last = np.minimum.accumulate(np.where(last_flag, at, N - 1)[:, ::-1], axis=1)[:, ::-1]      # ... and where it ends
    d_ranked = 2 * first + (last - first + 1) + 1
    d = np.empty((F, N), dtype=np.int64)
    np.put_along_axis(d, order, d_ranked, axis=1)
    return d - d.min(axis=1, keepdims=True)


def ranksum_inputs(a: np.ndarray, n1: int):
    """(planes, offsets, scales) of include/dcrx.h "association, rank-sum" from the a-matrix: planes[f, b] holds bit b of a[f, s]
    at bit s (uint64); offset = n1 A; scale = min(2^32 - 1, isqrt(2^64 // Q)), 0 where Q = 0 (all values equal), with A = sum a,
    B = sum a^2, Q = N B - A^2 (uint32 both)."""
    a = np.asarray(a, dtype=np.int64)
    F, N = a.shape
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << nat.ASSOC_RANKSUM_PLANES):
        raise ValueError("ranksum_inputs: a score outside 0 .. 127")
    planes = np.zeros((F, nat.ASSOC_RANKSUM_PLANES), dtype=np.uint64)
    for b in range(nat.ASSOC_RANKSUM_PLANES):
        for s in range(N):
            planes[:, b] |= ((a[:, s] >> b) & 1).astype(np.uint64) << np.uint64(s)
    A, B = a.sum(axis=1), (a * a).sum(axis=1)
    Q = N * B - A * A
    scale_of = {int(q): (min((1 << 32) - 1, isqrt((1 << 64) // int(q))) if q else 0) for q in np.unique(Q)}
    scales = np.array([scale_of[int(q)] for q in Q], dtype=np.uint32)
    return planes, (n1 * A).astype(np.uint32), scales


def ranksum_D(a: np.ndarray, case_mask: int, n1: int) -> np.ndarray:
    """D = N W - n1 A per feature (int64), W the sum of a over the cases."""
    a = np.asarray(a, dtype=np.int64)
    N = a.shape[1]
    cases = np.array([(case_mask >> s) & 1 for s in range(N)], dtype=np.int64)
    return N * (a * cases[None, :]).sum(axis=1) - n1 * a.sum(axis=1)


def ranksum_score(D: int, scale: int, alternative: str) -> int:
    """t of the contract, in Python integers."""
    u = D if alternative == "greater" else -D if alternative == "less" else abs(D)
    u = min(max(u, 0), (1 << nat.ASSOC_RANKSUM_SHIFT) - 1)
    return (u * scale) >> nat.ASSOC_RANKSUM_SHIFT


def z_text(D: int, Q: int, N: int, n1: int) -> str:
    return "nan" if Q == 0 else format(D * sqrt((N - 1) / (n1 * (N - n1) * Q)), ".6g")


def z_of_score(t: int, N: int, n1: int) -> float:
    """The z a score stands for, up to the rounding of scale: t = u 2^32 / (sqrt(Q) 2^20)."""
    return t / float(1 << (32 - nat.ASSOC_RANKSUM_SHIFT)) * sqrt((N - 1) / (n1 * (N - n1)))


def derive_ranksum(scores, edges, result, P: int) -> dict:
    """{"p_value", "p_adjusted": per feature of `scores` (the de-duplicated rows' observed scores spread back over the features is
    the caller's), here per distinct SCORE the Fraction (1 + #{p : perm_max[p] >= score}) / (P + 1); "O", "V", "fdr" (None where O
    is 0) and "q" per edge}."""
    most = np.sort(np.asarray(result["perm_max"], dtype=np.int64))
    p_adjusted = {int(t): Fraction(1 + len(most) - int(np.searchsorted(most, t, side="left")), P + 1) for t in set(int(x) for x in scores)}
    ranked = np.sort(np.asarray(scores, dtype=np.int64))
    E = len(edges)
    O, V, fdr, v = [0] * E, [0] * E, [None] * E, 0
    for j in range(E - 1, -1, -1):
        v += int(result["tail"][j])
        O[j] = len(ranked) - int(np.searchsorted(ranked, int(edges[j]), side="left"))
        V[j] = v
        fdr[j] = min(Fraction(1), Fraction(v, P * O[j])) if O[j] else None
    q, best = [None] * E, None
    for j in range(E):      # the smallest fdr over the edges at or below
        if fdr[j] is not None and (best is None or fdr[j] < best):
            best = fdr[j]
        q[j] = best
    return {"p_adjusted": p_adjusted, "O": O, "V": V, "fdr": fdr, "q": q}


def run_ranksum(inp: dict, features: dict, who: dict, path_in: str) -> dict:
    """The stage under --test rank-sum, from the cohort on."""
    from .io import write_out_associate
    alternative, P, seed = _get(inp, "alternative"), int(_get(inp, "permutations")), int(_get(inp, "seed"))
    min_count = int(_get(inp, "min_count"))
    N, n1 = len(who["used"]), who["n1"]
    if N > MAX_SAMPLES:
        raise ValueError(f"--test rank-sum takes 2 to {MAX_SAMPLES} samples with a group, not {N}: the wide form (up to {WIDE_MAX_SAMPLES} "
                         "samples, as the default test has) is not done")
    depths = None
    if inp.get("depths"):
        table = read_depths(inp["depths"], features["value"])
        for s in who["names"]:
            if s not in table:
                raise ValueError(f"{inp['depths']} (--depths): the sample {s!r} is used and has no row")
        depths = [table[s] for s in who["names"]]
        print(f"Ranking {features['value']} over the depths of {inp['depths']}")
    else:
        print(f"Ranking raw {features['value']}: no --depths, so a deeper sample ranks higher at the same frequency")
    a = rank_scores(features["values"], who["used"], min_count, depths, who["names"])
    F = len(a)
    planes, offsets, scales = ranksum_inputs(a, n1)
    D = ranksum_D(a, who["case_mask"], n1)
    A, B = a.sum(axis=1), (a * a).sum(axis=1)
    Q = N * B - A * A
    scores = np.array([ranksum_score(int(d), int(sc), alternative) for d, sc in zip(D, scales)], dtype=np.int64)
    if F:
        distinct, first, inverse, counts = np.unique(planes, axis=0, return_index=True, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
    else:
        distinct, first, inverse, counts = planes, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    levels = np.unique(scores)      # ascending
    edges = levels[-nat.ASSOC_RANKSUM_MAX_EDGES:].astype(np.uint32)
    result = derived = None
    if P:
        result = nat.assoc_ranksum(distinct, offsets[first], scales[first], counts.astype(np.uint32), N, who["case_mask"], alternative, edges, P, seed)
        if not np.array_equal(np.asarray(result["obs_score"], dtype=np.int64)[inverse], scores):
            raise RuntimeError("associate: the device's observed scores are not the host's")
        derived = derive_ranksum(scores, edges, result, P)
    masks = presence_masks(features["values"], who["used"], min_count)
    order = np.argsort(-scores, kind="stable")
    out_lines = ["\t".join(features["identity"] + RANKSUM_RESULT_COLUMNS).encode()]
    n0 = N - n1
    cell = np.searchsorted(edges.astype(np.int64), scores, side="right") - 1      # the largest edge at or below the score; -1: none
    for f in order:
        t, M = int(scores[f]), int(masks[f])
        zeros = int((a[f] == 0).sum())      # the samples of the smallest value: d = a + zeros + 1
        d_cases = sum(int(a[f, s]) + zeros + 1 for s in range(N) if who["case_mask"] >> s & 1)
        d_all = int(A[f]) + N * (zeros + 1)
        cells = [str(bin(M).count("1")), str(bin(M & who["case_mask"]).count("1")), str(bin(M & ~who["case_mask"]).count("1")), str(n1), str(n0),
                 format(d_cases / (2 * n1), ".6g"), format((d_all - d_cases) / (2 * n0), ".6g"), z_text(int(D[f]), int(Q[f]), N, n1), str(t)]
        if derived:
            cells += [sci(Fraction(1 + int(result["exceed"][inverse[f]]), P + 1)), sci(derived["p_adjusted"][t]),
                      sci(derived["q"][cell[f]] if cell[f] >= 0 else None)]
        else:
            cells += ["."] * 3
        out_lines.append(features["rows"][f] + b"\t" + "\t".join(cells).encode())
    out = {"result": result, "null": None}
    out["associate"] = write_out_associate(b"\n".join(out_lines) + b"\n", "associate.tsv", inp)
    if inp.get("write_null"):
        ranked = np.sort(scores)
        null = ["\t".join(RANKSUM_NULL_COLUMNS).encode()]
        for j in range(len(edges) - 1, -1, -1):
            e = int(edges[j])
            here = int(np.searchsorted(ranked, e, side="right") - np.searchsorted(ranked, e, side="left"))
            above = len(ranked) - int(np.searchsorted(ranked, e, side="left"))
            cells = [str(e), format(z_of_score(e, N, n1), ".6g"), str(here), str(above)]
            if derived:
                cells += [str(int(result["tail"][j])), str(derived["V"][j]), format(float(Fraction(derived["V"][j], P)), ".6g"), sci(derived["fdr"][j])]
            else:
                cells += ["."] * 4
            null.append("\t".join(cells).encode())
        out["null"] = write_out_associate(b"\n".join(null) + b"\n", "associate_null.tsv", inp)
    best = int(scores.max()) if F else None
    q05 = None
    if derived:
        q05 = sum(1 for j in cell if j >= 0 and derived["q"][j] is not None and derived["q"][j] <= Fraction(1, 20))
    stats.clear()
    stats.update({"test": "rank-sum", "kind": features["kind"], "value": features["value"], "samples": N, "cases": n1, "controls": n0,
                  "unknown": len(who["unknown"]), "not_in_ph": len(who["not_in_ph"]), "features": F, "rows": len(distinct), "permutations": P,
                  "seed": seed, "edges": len(edges), "depths": bool(depths), "max_score": best,
                  "min_p_adjusted": derived["p_adjusted"][best] if derived and F else None, "q_below_0.05": q05})
    out["stats"] = dict(stats)
    print(f"Associated {F:,} features ({len(distinct):,} distinct rows of scores; {features['kind']}, {features['value']} >= {min_count}, rank-sum) "
          f"with {inp['case']!r}: {N} samples used ({n1} cases, {n0} controls; {len(who['unknown'])} left out without a group, "
          f"{len(who['not_in_ph'])} without a row in -ph), {alternative}, {P:,} permutations, seed {seed}, {len(edges)} edges; largest score "
          f"{'.' if best is None else best}, smallest adjusted p {sci(stats['min_p_adjusted'])}, {'.' if q05 is None else q05} features with q <= 0.05")
    return out


# ---- what follows from the null ----

def derive(obs_rank, mult_of_rank, result, P: int, tail_ranks: int) -> dict:
    """{"p_adjusted": per RANK the Fraction (1 + #{p : perm_min[p] <= rank}) / (P + 1), "O", "V", "fdr" (None where O is 0) and
    "q" per tail rank}; obs_rank: the ranks that occur, mult_of_rank: the features at each rank (n_ranks entries)."""
    least = np.sort(np.asarray(result["perm_min"], dtype=np.int64))
    p_adjusted = {int(r): Fraction(1 + int(np.searchsorted(least, r, side="right")), P + 1) for r in set(int(x) for x in obs_rank)}
    O, V, fdr, o, v = [], [], [], 0, 0
    for r in range(tail_ranks):
        o += int(mult_of_rank[r])
        v += int(result["tail"][r])
        O.append(o); V.append(v)
        fdr.append(min(Fraction(1), Fraction(v, P * o)) if o else None)
    q, best = [None] * tail_ranks, None
    for r in range(tail_ranks - 1, -1, -1):
        if fdr[r] is not None and (best is None or fdr[r] < best):
            best = fdr[r]
        q[r] = best
    return {"p_adjusted": p_adjusted, "O": O, "V": V, "fdr": fdr, "q": q}


def odds_ratio(m: int, k: int, n1: int, n0: int) -> str:
    num, den = k * (n0 - m + k), (m - k) * (n1 - k)
    if den == 0:
        return "inf" if num else "nan"
    return format(float(Fraction(num, den)), ".6g")


def sci(x) -> str:
    return "." if x is None else format(float(x), ".6e")


def table_text(features: dict, m, k, ranks, who: dict, p_of_rank, derived, tail_ranks: int) -> bytes:
    out = ["\t".join(features["identity"] + RESULT_COLUMNS).encode()]
    n1, n0 = who["n1"], who["n0"]
    for f in np.argsort(ranks, kind="stable"):
        r, mf, kf = int(ranks[f]), int(m[f]), int(k[f])
        cells = [str(mf), str(kf), str(mf - kf), str(n1), str(n0), odds_ratio(mf, kf, n1, n0), sci(p_of_rank[r]),
                 sci(derived["p_adjusted"][r] if derived else None), sci(derived["q"][r] if derived and r < tail_ranks else None)]
        out.append(features["rows"][f] + b"\t" + "\t".join(cells).encode())
    return b"\n".join(out) + b"\n"


def null_text(p_of_rank, mult_of_rank, result, derived, P: int, tail_ranks: int) -> bytes:
    out = ["\t".join(NULL_COLUMNS).encode()]
    o = 0
    for r in range(tail_ranks):
        o += int(mult_of_rank[r])
        cells = [str(r), sci(p_of_rank[r]), str(int(mult_of_rank[r])), str(o)]
        if derived:
            cells += [str(int(result["tail"][r])), str(derived["V"][r]), format(float(Fraction(derived["V"][r], P)), ".6g"), sci(derived["fdr"][r])]
        else:
            cells += ["."] * 4
        out.append("\t".join(cells).encode())
    return b"\n".join(out) + b"\n"


def run(inp: dict) -> dict:
    """The stage: refusals, the two files, the cohort, the table of ranks, ONE permutation null on the GPU (none with
    --permutations 0), the derived columns and the files.  Returns {"associate": name, "null": name or None, "result": the native
    call's (None without permutations), "stats": {...}}.  ValueError for what refusal(), read_features(), read_phenotype() and
    cohort() name."""
    from .io import write_out_associate
    why = refusal(inp)
    if why:
        raise ValueError(why)
    alternative, P, seed = _get(inp, "alternative"), int(_get(inp, "permutations")), int(_get(inp, "seed"))
    max_p, min_count = parse_max_p(_get(inp, "max_p")), int(_get(inp, "min_count"))
    paths = infiles(inp)
    path_in = paths[0] if len(paths) == 1 else ", ".join(str(p) for p in paths)
    features = join_features(paths, inp.get("value"))
    groups = read_phenotype(inp["phenotype"], _get(inp, "ph_sample_column"), _get(inp, "ph_group_column"))
    who = cohort(features, groups, inp["case"], path_in, inp["phenotype"])
    for s in who["not_in_ph"]:
        print(f"Sample {s} of {path_in} has no row in {inp['phenotype']}: left out")
    if inp.get("test") == "rank-sum":
        return run_ranksum(inp, features, who, path_in)
    N, n1 = len(who["used"]), who["n1"]
    wide = N > MAX_SAMPLES      # 2 .. 64 samples: the narrow entry and everything as it was; 65 .. 1024: the wide one
    if wide and N > ANNOUNCE_TABLE_ABOVE:
        print(f"Building the table of exact p-values for {N} samples ({n1} cases): seconds on one CPU thread ...", flush=True)
    table, p_of_rank = (rank_table_sums if wide else rank_table)(N, n1, alternative)
    n_ranks = len(p_of_rank)
    tail_ranks = sum(p <= max_p for p in p_of_rank)
    if wide:
        masks = presence_words(features["values"], who["used"], min_count)
        F = len(masks)
        m, k = popcount_rows(masks), popcount_rows(masks & case_words(who["case_mask"], N)[None, :])
    else:
        masks = presence_masks(features["values"], who["used"], min_count)
        F = len(masks)
        m = np.array([bin(int(x)).count("1") for x in masks], dtype=np.int64)
        k = np.array([bin(int(x) & who["case_mask"]).count("1") for x in masks], dtype=np.int64)
    ranks = table[m, k].astype(np.int64) if F else np.zeros(0, np.int64)
    mult_of_rank = np.bincount(ranks, minlength=n_ranks)
    if wide and F:      # distinct rows, handed over in ascending popcount: the walk's runs of equal popcount are then one a slice
        distinct, inverse, counts = np.unique(masks, axis=0, return_inverse=True, return_counts=True)
        order = np.argsort(popcount_rows(distinct), kind="stable")
        place = np.empty(len(order), dtype=np.int64)
        place[order] = np.arange(len(order))
        distinct, counts, inverse = distinct[order], counts[order], place[inverse.reshape(-1)]
    elif wide:
        distinct, inverse, counts = masks, np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        distinct, inverse, counts = np.unique(masks, return_inverse=True, return_counts=True)
    result = derived = None
    if P:
        if wide:
            result = nat.assoc_permute_wide(distinct, counts.astype(np.uint32), N, case_words(who["case_mask"], N), table, n_ranks, tail_ranks,
                                            P, seed)
        else:
            result = nat.assoc_permute(distinct, counts.astype(np.uint32), N, who["case_mask"], table, n_ranks, tail_ranks, P, seed)
        if not np.array_equal(np.asarray(result["obs_rank"], dtype=np.int64)[inverse.reshape(-1)], ranks):
            raise RuntimeError("associate: the device's observed ranks are not the table's")
        derived = derive(ranks, mult_of_rank, result, P, tail_ranks)
    out = {"result": result, "null": None}
    out["associate"] = write_out_associate(table_text(features, m, k, ranks, who, p_of_rank, derived, tail_ranks), "associate.tsv", inp)
    if inp.get("write_null"):
        out["null"] = write_out_associate(null_text(p_of_rank, mult_of_rank, result, derived, P, tail_ranks), "associate_null.tsv", inp)
    best = int(ranks.min()) if F else None
    q05 = sum(int(mult_of_rank[r]) for r in range(tail_ranks) if derived and derived["q"][r] is not None and derived["q"][r] <= Fraction(1, 20))
    stats.clear()
    stats.update({"kind": features["kind"], "value": features["value"], "samples": N, "cases": n1, "controls": N - n1,
                  "unknown": len(who["unknown"]), "not_in_ph": len(who["not_in_ph"]), "features": F, "masks": len(distinct),
                  "permutations": P, "seed": seed, "n_ranks": n_ranks, "tail_ranks": tail_ranks,
                  "min_p": p_of_rank[best] if F else None, "min_p_adjusted": derived["p_adjusted"][best] if derived and F else None,
                  "q_below_0.05": q05 if derived else None})
    out["stats"] = dict(stats)
    print(f"Associated {F:,} features ({len(distinct):,} distinct presence patterns; {features['kind']}, {features['value']} >= {min_count}) "
          f"with {inp['case']!r}: {N} samples used ({n1} cases, {N - n1} controls; {len(who['unknown'])} left out without a group, "
          f"{len(who['not_in_ph'])} without a row in -ph), {alternative}, {P:,} permutations, seed {seed}, {tail_ranks} of {n_ranks} ranks "
          f"at or below {_get(inp, 'max_p')}; smallest p {sci(stats['min_p'])}, smallest adjusted p {sci(stats['min_p_adjusted'])}, "
          f"{'.' if not derived else q05} features with q <= 0.05")
    return out
