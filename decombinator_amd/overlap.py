"""The `overlap` sub-command: which clonotypes several samples share, and how alike two repertoires are.

Every path of this build ends in a `.clonotypes.tsv` (one row per v_call, j_call, junction_aa with its reads).  This stage
reads 1 to 64 of them, one per sample, and makes ONE call of _native.overlap (include/dcrx.h "overlap": the rows grouped by
(class, junction_aa bytes) on the GPU, the S x S matrices of what every two samples share, the public rows).  The reference
has no counterpart; there is no CPU fallback.

    python -m decombinator_amd overlap -in A.clonotypes.tsv B.clonotypes.tsv.gz ... [-op DIR] [-pf PREFIX] [-dz]
           [--overlap-key vj|v|none] [--min-samples N] [--downsample N|min [--seed INT]] [--diversity]

writes `<prefix>overlap_pairs.tsv[.gz]` — one line per pair of samples a < b in file order: their clonotypes and reads, what
they share, and four indices computed from those integers as exact fractions (Jaccard s / (n_a + n_b - s), the overlap
coefficient s / min(n_a, n_b), the Bray-Curtis similarity 2 sum min(w_a, w_b) / (X_a + X_b) and Morisita-Horn
2 sum w_a w_b X_a X_b / (sum w_a^2 X_b^2 + sum w_b^2 X_a^2); `nan` on a zero denominator) — and
`<prefix>overlap_public.tsv[.gz]` — the clonotypes at least --min-samples samples hold, with each sample's reads.
The class of a row is numbered over all files from its v_call / j_call STRINGS (vj: the pair, v: the V call, none: 0): no
gene set and no -tfdir are needed.

--downsample N|min first subsamples every sample's reads without replacement to one depth (N, or with `min` the reads of the
smallest sample that has any) by ONE call of _native.downsample (include/dcrx.h "downsample": a counter-based key per read,
the n smallest keys of a sample are kept; --seed, 1 by default, picks the keys) over the rows in file order, before anything
is grouped: a row's reads become its kept reads, a row that keeps none is dropped, a sample with fewer reads than the depth
is kept whole.  --diversity writes `<prefix>overlap_diversity.tsv[.gz]`, one line per sample in file order, computed on the
host from the sample's abundance classes (_native.abundance_classes over the groups of the overlap call): reads before
downsampling and after, clonotypes R, singletons f1, doubletons f2, the largest clonotype, D50 (the fewest clonotypes, largest
first, that hold half the reads), Chao1 R + f1 (f1 - 1) / (2 (f2 + 1)), Simpson sum w (w - 1) / (X (X - 1)), inverse Simpson
X^2 / sum w^2, the Gini coefficient, Shannon's entropy (natural logarithm) and clonality 1 - H / ln R; `nan` where a
denominator is zero."""
from __future__ import annotations

import gzip
import math
import os
from fractions import Fraction

import numpy as np

from . import _native as nat

SUFFIXES = (".clonotypes.tsv.gz", ".clonotypes.tsv")
KEYS = ("vj", "v", "none")
HEADER = "\t".join(nat.CLONOTYPE_COLUMNS).encode()

stats: dict = {}      # the statistics of the last run()


def sample_name(path: str) -> str:
    """The file's name without its directory and without `.clonotypes.tsv[.gz]`."""
    base = os.path.basename(str(path))
    for suffix in SUFFIXES:
        if base.endswith(suffix):
            return base[:-len(suffix)]
    return base


def refusal(inp: dict):
    """Why these arguments cannot run, or None — decided before any file is opened."""
    files = list(inp.get("infile") or [])
    if not 1 <= len(files) <= nat.OVERLAP_MAX_SAMPLES:
        return f"overlap takes 1 to {nat.OVERLAP_MAX_SAMPLES} .clonotypes.tsv files (-in), not {len(files)}"
    names = [sample_name(f) for f in files]
    for k, name in enumerate(names):
        if name in names[:k]:
            return f"two files give one sample name ({name!r}): {files[names.index(name)]} and {files[k]}"
    min_samples = inp.get("min_samples", 2)
    if not 1 <= min_samples <= len(files):
        return f"--min-samples is 1 .. the number of files ({len(files)}), not {min_samples}"
    if inp.get("overlap_key", "vj") not in KEYS:
        return f"--overlap-key is vj, v or none, not {inp['overlap_key']}"
    depth, seed = inp.get("downsample"), inp.get("seed")
    if depth is not None and downsample_depth(depth) is None:
        return f"--downsample is a number of reads (1 or more) or min, not {depth!r}"
    if seed is not None:
        if depth is None:
            return "--seed picks the subsample of --downsample: it is refused without it"
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            return f"--seed is 0 .. 2^64 - 1, not {seed!r}"
    return None


def downsample_depth(value):
    """--downsample's value: "min", an integer >= 1, or None for anything else."""
    if isinstance(value, bool):
        return None
    if isinstance(value, int):
        return value if value >= 1 else None
    text = str(value).strip()
    if text == "min":
        return "min"
    if text.isascii() and text.isdigit() and int(text) >= 1:
        return int(text)
    return None


def read_table(path: str):
    """The rows of one `.clonotypes.tsv` (plain or .gz): lists of v_call, j_call (str), junction_aa (bytes) and
    duplicate_count (int).  The header line must be the clonotype table's."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if not lines or lines[0].rstrip(b"\r") != HEADER:
        raise ValueError(f"{path} is not a .clonotypes.tsv: its first line is not {HEADER.decode()!r}")
    v, j, aa, dup = [], [], [], []
    for n, line in enumerate(lines[1:], 2):
        f = line.split(b"\t")
        if len(f) < 4:
            raise ValueError(f"{path}, line {n}: fewer than four columns")
        try:
            count = int(f[3])
        except ValueError:
            raise ValueError(f"{path}, line {n}: duplicate_count {f[3]!r} is not a number") from None
        if count < 0:
            raise ValueError(f"{path}, line {n}: duplicate_count {count} is negative")
        v.append(f[0].decode("latin-1")); j.append(f[1].decode("latin-1")); aa.append(f[2]); dup.append(count)
    return v, j, aa, dup


def index_fraction(num: int, den: int) -> str:
    """num / den as an exact fraction, then six decimals; nan on a zero denominator."""
    return format(float(Fraction(num, den)), ".6f") if den else "nan"


def pairs_text(names, result: dict) -> bytes:
    """The `overlap_pairs.tsv` text from the planes: one line per a < b."""
    P = {k: result[k] for k in nat.OVERLAP_PLANES}

    def product(a, b):
        return (int(P["prod_hi"][a][b]) << 32) + int(P["prod_lo"][a][b])
    lines = ["\t".join(nat.OVERLAP_PAIR_COLUMNS)]
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            n_a, n_b, s = int(P["shared"][a][a]), int(P["shared"][b][b]), int(P["shared"][a][b])
            x_a, x_b = int(P["shared_weight"][a][a]), int(P["shared_weight"][b][b])
            low = int(P["min_weight"][a][b])
            lines.append("\t".join([
                names[a], names[b], str(n_a), str(n_b), str(s), str(x_a), str(x_b), str(int(P["shared_weight"][a][b])),
                str(int(P["shared_weight"][b][a])), str(low),
                index_fraction(s, n_a + n_b - s), index_fraction(s, min(n_a, n_b)), index_fraction(2 * low, x_a + x_b),
                index_fraction(2 * product(a, b) * x_a * x_b, product(a, a) * x_b * x_b + product(b, b) * x_a * x_a)]))
    return ("\n".join(lines) + "\n").encode("utf-8", "surrogateescape")


def diversity_text(names, reads_in, classes: dict) -> bytes:
    """The `overlap_diversity.tsv` text: one line per sample from its abundance classes (class_off, class_count, class_mult:
    the distinct clonotype sizes ascending, and how many clonotypes have each) and nothing else."""
    off = [int(x) for x in classes["class_off"]]
    lines = ["\t".join(nat.OVERLAP_DIVERSITY_COLUMNS)]
    for s, name in enumerate(names):
        cls = [(int(classes["class_count"][k]), int(classes["class_mult"][k])) for k in range(off[s], off[s + 1])]
        X, R = sum(c * k for c, k in cls), sum(k for _, k in cls)
        f1, f2 = (sum(k for c, k in cls if c == want) for want in (1, 2))
        d50, held = 0, 0
        for c, k in reversed(cls):      # largest first: the clonotypes of this size that are still needed
            need = -(-(X - 2 * held) // (2 * c))
            if need <= k:
                d50 += max(need, 0)
                break
            d50, held = d50 + k, held + c * k
        gini, below = 0, 0              # the clonotypes of a class take the ranks below + 1 .. below + k
        for c, k in cls:
            gini += c * k * (2 * below + k - R)
            below += k
        shannon = math.fsum(k * (c / X) * math.log(X / c) for c, k in cls) + 0.0 if X else 0.0
        lines.append("\t".join([
            name, str(int(reads_in[s])), str(X), str(R), str(f1), str(f2), str(max((c for c, _ in cls), default=0)), str(d50),
            index_fraction(2 * R * (f2 + 1) + f1 * (f1 - 1), 2 * (f2 + 1)),
            index_fraction(sum(c * (c - 1) * k for c, k in cls), X * (X - 1)),
            index_fraction(X * X, sum(c * c * k for c, k in cls)),
            index_fraction(gini, R * X),
            format(shannon, ".6f"),
            format(1.0 - shannon / math.log(R), ".6f") if R >= 2 else "nan"]))
    return ("\n".join(lines) + "\n").encode("utf-8", "surrogateescape")


def run(inp: dict) -> dict:
    """The stage: refusals, the files, (the subsample,) the one call, the statistics line, the files.  Returns {"pairs": name,
    "public": name, "result": ..., "stats": ...}, with --diversity "diversity": name and with --downsample "downsample": what
    was kept.  ValueError for what refusal() names and for a file that is no clonotype table."""
    from .io import write_out_overlap
    why = refusal(inp)
    if why:
        raise ValueError(why)
    files = list(inp["infile"])
    names = [sample_name(f) for f in files]
    mode = inp.get("overlap_key", "vj")
    class_key = {"vj": lambda v, j: (v, j), "v": lambda v, j: v, "none": lambda v, j: None}[mode]
    v_no, j_no, class_no = {}, {}, {}
    samples, classes, v_idx, j_idx, strings, weights = [], [], [], [], [], []
    for s, path in enumerate(files):
        v, j, aa, dup = read_table(path)
        for k in range(len(v)):
            samples.append(s)
            classes.append(class_no.setdefault(class_key(v[k], j[k]), len(class_no)))
            v_idx.append(v_no.setdefault(v[k], len(v_no)))
            j_idx.append(j_no.setdefault(j[k], len(j_no)))
        strings += aa
        weights += dup
    reads_in = [0] * len(files)
    for a, w in zip(samples, weights):
        reads_in[a] += w
    out = {}
    if inp.get("downsample") is not None:
        depth = downsample_depth(inp["downsample"])
        if depth == "min":
            depth = min((x for x in reads_in if x), default=0)
        seed = 1 if inp.get("seed") is None else int(inp["seed"])
        for name, x in zip(names, reads_in):
            if x < depth:
                print(f"Sample {name} has {x:,} reads, fewer than {depth:,}: it is kept whole")
        sub = nat.downsample(np.array(samples, dtype=np.uint32), np.array(weights, dtype=np.uint64), len(files),
                             np.full(len(files), depth, dtype=np.uint64), seed)
        kept = [int(x) for x in sub["kept"]]
        rows = [k for k in range(len(kept)) if kept[k]]
        dropped = [0] * len(files)
        for k in range(len(kept)):
            dropped[samples[k]] += not kept[k]
        print(f"Downsampled to {depth:,} reads per sample (seed {seed}): " + "; ".join(
            f"{name} {reads_in[a]:,} reads in, {int(sub['depth_used'][a]):,} kept, {dropped[a]:,} rows dropped" for a, name in enumerate(names)))
        samples, classes, v_idx, j_idx, strings = ([col[k] for k in rows] for col in (samples, classes, v_idx, j_idx, strings))
        weights = [kept[k] for k in rows]
        out["downsample"] = {"depth": depth, "seed": seed, "reads_in": reads_in, "depth_used": [int(x) for x in sub["depth_used"]],
                             "rows_dropped": dropped}
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        off[1:] = np.cumsum([len(b) for b in strings])
    text = b"".join(strings)
    result, st = nat.overlap(np.array(samples, dtype=np.uint32), np.array(classes, dtype=np.uint32), off, text,
                             np.array(weights, dtype=np.uint64), len(files), int(inp.get("min_samples", 2)))
    stats.clear()
    stats.update(st)
    print(f"Overlap of {len(files)} samples ({mode}): {st['rows_in']:,} rows in, {st['groups']:,} clonotypes, {st['private_groups']:,} "
          f"in one sample, {st['shared_groups']:,} in two or more, {st['in_all_samples']:,} in all (at most {st['largest_n_samples']} "
          f"samples hold one); {st['public_rows']:,} public rows with {st['public_cells']:,} cells")
    public = nat.format_overlap_public(result, names, v_idx, j_idx, list(v_no), list(j_no), off, text)
    out.update(result=result, stats=st)
    out["pairs"] = write_out_overlap(pairs_text(names, result), "overlap_pairs.tsv", inp)
    out["public"] = write_out_overlap(public, "overlap_public.tsv", inp)
    if inp.get("diversity"):
        classes = nat.abundance_classes(np.array(samples, dtype=np.uint32), np.asarray(result["group_of"], dtype=np.uint32),
                                        np.array(weights, dtype=np.uint64), len(files))
        out["diversity"] = write_out_overlap(diversity_text(names, reads_in, classes), "overlap_diversity.tsv", inp)
    return out
