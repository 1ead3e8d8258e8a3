"""Helpers of the stage-2 collapse tests (test_collapse_cluster.py, test_gpu_collapse_cluster.py): an independent neighbour
search (plain Levenshtein DP, no code shared with the kernel) and the fixture cases of tests/golden/collapse_cluster.json
(made by tests/golden_gen/gen_collapse_cluster.py from the reference's own collapsinator)."""
import functools
import gzip
import hashlib
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def lev(a, b):
    """Levenshtein distance, the textbook DP."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def lev_many(a, b):
    """The same DP over many pairs at once (numpy, one row of the table per step): a, b lists of equal length."""
    n = len(a)
    la = np.array([len(x) for x in a], dtype=np.int32)
    lb = np.array([len(x) for x in b], dtype=np.int32)
    ma, mb = int(la.max(initial=0)), int(lb.max(initial=0))
    A = np.full((n, ma), -1, dtype=np.int32)
    B = np.full((n, mb), -2, dtype=np.int32)
    for q, x in enumerate(a):
        A[q, :len(x)] = np.frombuffer(x.encode("latin-1"), dtype=np.uint8)
    for q, x in enumerate(b):
        B[q, :len(x)] = np.frombuffer(x.encode("latin-1"), dtype=np.uint8)
    prev = np.tile(np.arange(mb + 1, dtype=np.int32), (n, 1))
    out = np.where(la == 0, lb, 0)
    for i in range(1, ma + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        sub = (A[:, i - 1:i] != B).astype(np.int32)
        diag = prev[:, :-1] + sub
        up = prev[:, 1:] + 1
        best = np.minimum(diag, up)
        for j in range(1, mb + 1):
            cur[:, j] = np.minimum(best[:, j - 1], cur[:, j - 1] + 1)
        prev = cur
        done = la == i
        out[done] = prev[done, lb[done]]
    return out


def _as_list(umis):
    if isinstance(umis, tuple):
        t, o = umis
        return [t[int(o[i]):int(o[i + 1])].decode("latin-1") for i in range(len(o) - 1)]
    return [u if isinstance(u, str) else bytes(u).decode("latin-1") for u in umis]


def brute_neighbours(umis, k):
    """Every (i, j), i < j, within distance k, ascending — length and composition prefilters (both exact lower bounds) in
    numpy, the DP on what is left.  Same signature as _native.umi_neighbours."""
    umis = _as_list(umis)
    n = len(umis)
    if n < 2:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    alphabet = sorted(set("".join(umis))) or ["A"]
    comp = np.array([[u.count(c) for c in alphabet] for u in umis], dtype=np.int64).reshape(n, len(alphabet))
    lens = np.array([len(u) for u in umis], dtype=np.int64)
    ci, cj = [], []
    for i in range(n - 1):
        j = np.arange(i + 1, n)
        ok = (np.abs(lens[j] - lens[i]) <= k) & (np.abs(comp[j] - comp[i]).sum(axis=1) <= 2 * k)
        ci.append(np.full(int(ok.sum()), i, dtype=np.int64))
        cj.append(j[ok].astype(np.int64))
    ci, cj = np.concatenate(ci), np.concatenate(cj)
    keep = np.zeros(len(ci), dtype=bool)
    for s in range(0, len(ci), 200000):
        e = min(len(ci), s + 200000)
        keep[s:e] = lev_many([umis[x] for x in ci[s:e].tolist()], [umis[x] for x in cj[s:e].tolist()]) <= k
    return ci[keep], cj[keep]


SPACERS = {"m13": ("GTCGTGACTGGGAAAACCCTGG", "GTCGTGAT"), "i8_single": ("ATCACGAC", None)}


def rnd(rng, k, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(k))


def mutate(rng, s, kind):
    s = list(s)
    i = rng.randrange(len(s))
    if kind == "sub":
        s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    elif kind == "ins":
        s.insert(i, rng.choice("ACGT"))
    else:
        del s[i]
    return "".join(s)


def synth_rows(seed, oligo, n_rows, allow_n):
    """Synthetic `.n12` rows of a fixture case (the generator and the tests make the same ones from the seed).  Molecules (a UMI and a TCR), each read a few times; some reads carry a seq error (ties, re-keys), some a UMI error
    (substitution or indel in either half: neighbouring UMIs, lengths that vary), some barcodes are reused by another TCR
    (multi-TCR), and DCRs repeat across molecules (cluster votes, ties, means of .5)."""
    rng = random.Random(seed)
    s1, s2 = SPACERS[oligo]
    dcrs = [(str(rng.randrange(40)), str(rng.randrange(12)), str(rng.randrange(6)), str(rng.randrange(6)), rnd(rng, rng.randrange(0, 5)))
            for _ in range(300)]
    rows = []
    while len(rows) < n_rows:
        h1, h2 = rnd(rng, 6), rnd(rng, 6)
        family = [(h1, h2)]
        for _ in range(rng.choice([0, 0, 1, 2, 4, 6, 8])):                          # UMI errors of the same molecule
            a, b = rng.choice(family)
            if rng.random() < 0.5:
                a = mutate(rng, a, rng.choice(["sub", "sub", "ins", "del"]))
            else:
                b = mutate(rng, b, rng.choice(["sub", "sub", "sub", "del"]))
            family.append((a, b))
        dcr = rng.choice(dcrs)
        seq = rnd(rng, rng.randrange(28, 40))
        for a, b in family:
            if allow_n and rng.random() < 0.05:
                a = a[:2] + "N" + a[3:]
            n_reads = rng.choice([1, 1, 2, 2, 3, 4])
            for r in range(n_reads):
                sq = seq
                if rng.random() < 0.25:
                    sq = mutate(rng, seq, rng.choice(["sub", "sub", "ins", "del"]))
                if rng.random() < 0.03:                                               # another TCR on this barcode
                    sq = rnd(rng, len(seq))
                d = dcr if rng.random() < 0.93 else rng.choice(dcrs)
                if oligo == "m13":
                    region = rnd(rng, rng.choice([0, 0, 1, 2])) + s1 + a + s2 + b + rnd(rng, 6)
                else:
                    region = a + s1 + b + rnd(rng, 4)
                qual = "".join(chr(33 + rng.choice([40] * 14 + [30, 12])) for _ in region)
                rows.append(", ".join(list(d) + [f"r{len(rows)}", sq, "I" * len(sq), region, qual]))
    return rows[:n_rows]


def cases():
    return json.load(open(os.path.join(GOLDEN, "collapse_cluster.json")))["cases"]


def case_rows(case):
    p = case["params"]
    return ("\n".join(synth_rows(p["seed"], p["oligo"].lower(), p["n_rows"], p["allowNs"])) + "\n").encode()


def run_case(case, workdir, via_cli=False):
    """Runs one fixture case in `workdir` (the working directory: -bd and -wc write there) and returns what it wrote."""
    from decombinator_amd import collapse, pipeline
    from decombinator_amd import io as dio
    p = case["params"]
    (workdir / "dcr_CASE_1_beta.n12").write_bytes(case_rows(case))
    argv = ["collapse", "-in", "dcr_CASE_1_beta.n12", "-c", "b", "--cluster", "-dz", "-dc", "-ol", p["oligo"],
            "-bc", str(p["bcthreshold"]), "-lv", str(p["percentlevdist"]), "-di"]
    if p["allowNs"]:
        argv.append("-N")
    if case["extra"]:
        argv += ["-bd", "-uh", "-wc"]
    if via_cli:
        pipeline.main(argv)
        freq = (workdir / "dcr_CASE_1_beta.freq").read_text().splitlines()
    else:
        inp = dio.cli_args(argv)
        freq = [", ".join(map(str, r)) for r in collapse.collapsinator(inp)]
    logs = sorted(os.listdir(workdir / "Logs"))
    summary = (workdir / "Logs" / [x for x in logs if "Collapsing_Summary" in x][-1]).read_text()
    out = {"freq": freq, "summary_body": summary.split("\n\n", 1)[1], "counts": dict(collapse.counts)}
    if case["extra"]:
        out["bd"] = (workdir / "dcr_CASE_1_beta_barcode_duplication.txt").read_bytes()
        out["uh"] = (workdir / "Logs" / [x for x in logs if "UMIhistogram" in x][-1]).read_text()
        out["wc"] = gzip.open(workdir / "clusters_b.psv.gz", "rb").read()
    return out


def check_case(case, got):
    assert got["freq"] == case["freq"]
    assert got["summary_body"] == case["summary_body"]
    for k, v in case["counts"].items():
        if k.startswith("pc_") or k.startswith("avg_"):
            continue                       # derived by the summary writer from the keys below
        assert got["counts"].get(k, 0) == v, k
    if case["extra"]:
        assert hashlib.sha256(got["bd"]).hexdigest() == case["bd_sha256"]
        assert got["uh"] == case["uh"]
        assert hashlib.sha256(got["wc"]).hexdigest() == case["wc_sha256"]


def symdel_neighbours(umis, k):
    """Every (i, j), i < j, within distance k, ascending, for large lists: candidates are the pairs that share a string
    reachable by at most k deletions from each (every pair within k does), each decided by the DP (lev_many)."""
    from itertools import combinations
    umis = _as_list(umis)
    by_variant = {}
    for i, u in enumerate(umis):
        seen = set()
        for d in range(min(k, len(u)) + 1):
            for pos in combinations(range(len(u)), d):
                v = "".join(c for p, c in enumerate(u) if p not in pos)
                if v not in seen:
                    seen.add(v)
                    by_variant.setdefault(v, []).append(i)
    keys = set()
    for lst in by_variant.values():
        if len(lst) > 1:
            for a in range(len(lst)):
                for b in range(a + 1, len(lst)):
                    keys.add((lst[a] << 32) | lst[b])
    cand = np.array(sorted(keys), dtype=np.int64)
    ci, cj = cand >> 32, cand & 0xFFFFFFFF
    keep = np.zeros(len(cand), dtype=bool)
    for s in range(0, len(cand), 200000):
        e = min(len(cand), s + 200000)
        keep[s:e] = lev_many([umis[x] for x in ci[s:e].tolist()], [umis[x] for x in cj[s:e].tolist()]) <= k
    return ci[keep], cj[keep]


# ---- constructed UMI lists for the neighbour search (dcrx_umi.hip): each one puts a mechanism of the kernel's tile walk on
# the spot (test_collapse_cluster.py on the host, test_gpu_collapse_cluster.py on the device).  Every list comes shuffled
# with a fixed seed, so original indices differ from sorted positions. ----

UMI_SYMBOLS = "ACGTNSL\xff"
UMI_TILE = 256
K_HUGE = (2 ** 30, 2 ** 31 - 1)


def _shuffled(umis, seed):
    umis = list(umis)
    random.Random(seed).shuffle(umis)
    return umis


@functools.lru_cache(maxsize=None)
def umi_all_pairs_list():
    """600 distinct UMIs of lengths 0-24 (the empty one among them) over eight byte values: three tiles (256, 256, 88); at
    k = 24 every pair is a neighbour, so every ballot of a full wave has 64 hits."""
    rng = random.Random(600)
    seen = {"": None}
    while len(seen) < 600:
        seen["".join(rng.choice(UMI_SYMBOLS) for _ in range(rng.randrange(1, 25)))] = None
    return tuple(_shuffled(seen, 601))


@functools.lru_cache(maxsize=None)
def umi_ball_list():
    """A 24-mer over the eight symbols and its 168 single substitutions: at k = 2 all 14 196 pairs, at k = 1 the 168 with
    the centre and the 24 * 21 that share a position."""
    rng = random.Random(24)
    centre = list(UMI_SYMBOLS * 3)
    rng.shuffle(centre)
    out = ["".join(centre)]
    for p in range(24):
        out += ["".join(centre[:p] + [c] + centre[p + 1:]) for c in UMI_SYMBOLS if c != centre[p]]
    return tuple(_shuffled(out, 25))


@functools.lru_cache(maxsize=None)
def umi_family_list(n=1300, seed=9):
    """Families with the length limits in them: base lengths from {0, 1, 2, 11, 12, 13, 23, 24}, members by substitutions
    (N included), insertions, deletions and exact repeats; not distinct.  The first n of the generator's list, shuffled."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        base = "".join(rng.choice("ACGT") for _ in range(rng.choice([0, 1, 2, 11, 11, 12, 12, 12, 13, 13, 23, 23, 24, 24, 24])))
        fam = [base]
        for _ in range(rng.choice([0, 1, 2, 4, 6])):
            s = list(rng.choice(fam))
            for _ in range(rng.randrange(0, 3)):                    # no edit at all: an exact repeat
                op = rng.randrange(4)
                if op < 2 and s:
                    s[rng.randrange(len(s))] = rng.choice("ACGTN")
                elif op == 2 and len(s) < 24:
                    s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
                elif s:
                    del s[rng.randrange(len(s))]
            fam.append("".join(s))
        out += fam
    return tuple(_shuffled(out[:n], seed + 1))


@functools.lru_cache(maxsize=None)
def umi_reach_len_list(k):
    """256 distinct 10-mers, the same with k symbols appended, and 256 unrelated 24-mers: tiles 0 and 1 are k apart in length
    and 256 pairs at distance k cross them."""
    rng = random.Random(100 + k)
    short = {}
    while len(short) < 256:
        short[rnd(rng, 10)] = None
    far = {}
    while len(far) < 256:
        far[rnd(rng, 24)] = None
    return tuple(_shuffled(list(short) + [u + rnd(rng, k) for u in short] + list(far), 110 + k))


@functools.lru_cache(maxsize=None)
def umi_reach_comp_list(k):
    """256 distinct 12-mers of one composition (3 each of A, C, G, T) and the same with their first k A's turned into N, a
    symbol the first group lacks: two tiles of one length, 2k apart in composition (k fewer A, k more N), and 256 pairs at
    distance k cross them.  The first element is fixed (symbol codes follow first appearance: A, C, G, T, then N)."""
    rng = random.Random(200 + k)
    first = "AAACCCGGGTTT"
    plain = {first: None}
    while len(plain) < 256:
        s = list(first)
        rng.shuffle(s)
        plain["".join(s)] = None
    rest = _shuffled(list(plain)[1:] + [u.replace("A", "N", k) for u in plain], 210 + k)
    return tuple([first] + rest)


TILE_EDGE_N = (2, 255, 256, 257, 511, 512, 513)
TILE_EDGE_SEED = 9


def umi_constructed_cases():
    """(name, list, the k values its GPU test runs) of every constructed list."""
    cases = [("all_pairs", umi_all_pairs_list(), (24,) + K_HUGE), ("ball", umi_ball_list(), (1, 2)),
             ("families", umi_family_list(), (0, 1, 2, 3))]
    cases += [(f"families_{n}", umi_family_list(n, TILE_EDGE_SEED), (2,)) for n in TILE_EDGE_N]
    cases += [(f"reach_len_{k}", umi_reach_len_list(k), (k,)) for k in (1, 2)]
    cases += [(f"reach_comp_{k}", umi_reach_comp_list(k), (k,)) for k in (1, 2)]
    return cases


@functools.lru_cache(maxsize=None)
def brute_keys(umis, k):
    """brute_neighbours of a constructed list (a tuple) as sorted uint64 keys (i << 32 | j); computed once per (list, k).
    No two strings of at most 24 symbols are more than 24 edits apart, so a k above 24 has the pairs of k = 24."""
    assert max(len(u) for u in umis) <= 24
    if k > 24:
        return brute_keys(umis, 24)
    r, c = brute_neighbours(list(umis), k)
    keys = (r.astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64)
    keys.sort()
    keys.setflags(write=False)
    return keys
