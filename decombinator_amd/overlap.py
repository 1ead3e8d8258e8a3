"""The `overlap` sub-command: which clonotypes several samples share, and how alike two repertoires are.

Every path of this build ends in a `.clonotypes.tsv` (one row per v_call, j_call, junction_aa with its reads).  This stage
reads 1 to 64 of them, one per sample, and makes ONE call of _native.overlap (include/dcrx.h "overlap": the rows grouped by
(class, junction_aa bytes) on the GPU, the S x S matrices of what every two samples share, the public rows).  The reference
has no counterpart; there is no CPU fallback.

    python -m decombinator_amd overlap -in A.clonotypes.tsv B.clonotypes.tsv.gz ... [-op DIR] [-pf PREFIX] [-dz]
           [--overlap-key vj|v|none] [--min-samples N]

writes `<prefix>overlap_pairs.tsv[.gz]` — one line per pair of samples a < b in file order: their clonotypes and reads, what
they share, and four indices computed from those integers as exact fractions (Jaccard s / (n_a + n_b - s), the overlap
coefficient s / min(n_a, n_b), the Bray-Curtis similarity 2 sum min(w_a, w_b) / (X_a + X_b) and Morisita-Horn
2 sum w_a w_b X_a X_b / (sum w_a^2 X_b^2 + sum w_b^2 X_a^2); `nan` on a zero denominator) — and
`<prefix>overlap_public.tsv[.gz]` — the clonotypes at least --min-samples samples hold, with each sample's reads.
The class of a row is numbered over all files from its v_call / j_call STRINGS (vj: the pair, v: the V call, none: 0): no
gene set and no -tfdir are needed."""
from __future__ import annotations

import gzip
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


def run(inp: dict) -> dict:
    """The stage: refusals, the files, the one call, the statistics line, the two files.  Returns {"pairs": name,
    "public": name, "result": ..., "stats": ...}.  ValueError for what refusal() names and for a file that is no clonotype
    table."""
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
    out = {"result": result, "stats": st}
    out["pairs"] = write_out_overlap(pairs_text(names, result), "overlap_pairs.tsv", inp)
    out["public"] = write_out_overlap(public, "overlap_public.tsv", inp)
    return out
