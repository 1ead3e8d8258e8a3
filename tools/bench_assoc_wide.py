#!/usr/bin/env python3
"""The wide permutation null on the GPU (include/dcrx.h "association, wide"): one JSON line with, for seeded distinct presence
patterns of N samples, half of them cases — most features in 2 to 4 samples, one in a hundred dense (fair bits), a multiplicity
of 1 and more each, handed over in ascending popcount — and the table of the one-sided exact test (`greater`, built by
associate.rank_table_sums) with the ranks at or below --max-p as the tail:
  - dcrx_assoc_permute_wide_device (prepare, labels and permute kernels) under device events around the whole call: the median
    of --repeats after a warm-up, with the smallest and the largest, and the pairs a nanosecond;
  - dcrx_assoc_permute_wide, the host entry, by the wall clock (the allocation, the uploads and the copies back included);
  - at N = 64 the narrow entry (dcrx_assoc_permute_device) beside the wide one on the same masks: the first yardstick;
  - at --numpy-shape the numpy form of the wide contract on one thread, which the device's four arrays must equal: the second;
  - the shuffled order beside the ascending one at --shuffled (features x permutations x samples);
  - a dense case: ONE pattern everywhere and tail_ranks = n_ranks, so every (feature, relabeling) pair adds to a cell.
--out FILE rewrites the result so far after every shape.  --dry checks the arguments and builds the first patterns, and touches
no device.
Usage: tools/bench_assoc_wide.py [--samples 128,256,640,1024] [--features 100000,1000000] [--permutations 1000,10000]
                                 [--max-p 0.05] [--dense 100000x10000x640] [--shuffled 100000x10000x640]
                                 [--numpy-shape 2000x200x130] [--repeats 15] [--seed 1] [--dry] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decombinator_amd import _native as nat  # noqa: E402
from decombinator_amd import associate as asc  # noqa: E402
from bench_cdr3_profile import timed  # noqa: E402


SAMPLE_STEP, READ_STEP = 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15      # decombinator_amd/csrc/dcrx_rarefy_core.h: the steps of the key


def words_for(N):
    return (N + 63) // 64


def case_words(N):
    """Every other sample a case."""
    return asc.case_words(sum(1 << s for s in range(0, N, 2)), N)


def seeded_rows(N, F, seed):
    """F distinct presence patterns of N samples as F x W words, in ascending popcount, and their multiplicities: 99 in 100 in 2
    to 4 samples (drawn with replacement: a few fall below), one in a hundred N fair bits."""
    rng = np.random.default_rng(seed)
    W = words_for(N)
    have = np.zeros((0, W), np.uint64)
    while len(have) < F:
        n = F - len(have) + 1024
        m = rng.integers(2, 5, n)
        where = rng.integers(0, N, size=(n, 4))
        rows = np.zeros((n, W), np.uint64)
        for j in range(4):
            on = j < m
            np.bitwise_or.at(rows, (np.flatnonzero(on), where[on, j] >> 6), np.uint64(1) << (where[on, j] & 63).astype(np.uint64))
        dense = np.flatnonzero(rng.integers(0, 100, n) == 0)
        rows[dense] = rng.integers(0, 1 << 63, (len(dense), W), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (len(dense), W), dtype=np.uint64)
        rows[:, W - 1] &= np.uint64((1 << (N - 64 * (W - 1))) - 1 if N % 64 else (1 << 64) - 1)
        have = np.unique(np.concatenate([have, rows]), axis=0)
    have = rng.permutation(have)[:F]
    have = have[np.argsort(asc.popcount_rows(have), kind="stable")]
    return np.ascontiguousarray(have), rng.geometric(0.3, F).astype(np.uint32)


def numpy_permute_wide(masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed):
    """The wide contract in numpy, whole arrays at a time: labels by argsort of the keys, scores by popcounts over words."""
    u, W = np.uint64, words_for(N)
    n1 = int(asc.popcount_rows(np.asarray(cw, np.uint64)[None, :])[0])
    with np.errstate(over="ignore"):
        z = np.arange(1, P + 1, dtype=np.uint64) * u(SAMPLE_STEP) + u(seed)
        for rounds in range(2):
            for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
                z ^= z >> u(shift)
                z *= u(mul)
            z ^= z >> u(31)
            if rounds == 0:
                z = z[:, None] + np.arange(1, N + 1, dtype=np.uint64)[None, :] * u(READ_STEP)
    first = np.argsort(z, axis=1, kind="stable")[:, :n1]
    L = np.zeros((P, W), np.uint64)
    for p in range(P):
        np.bitwise_or.at(L[p], first[p] >> 6, u(1) << (first[p] & 63).astype(np.uint64))
    table = np.asarray(table, np.uint32).reshape(-1)
    m = asc.popcount_rows(masks)
    obs = table[m * (N + 1) + asc.popcount_rows(masks & np.asarray(cw, np.uint64)[None, :])]
    least, tail = np.full(P, n_ranks, np.uint32), np.zeros(tail_ranks, np.uint64)
    part = mults > 0
    mk, w, row = masks[part], mults[part].astype(np.float64), m[part] * (N + 1)
    for p in range(P):
        r = table[row + asc.popcount_rows(mk & L[p][None, :])].astype(np.int64)
        least[p] = r.min() if len(r) else n_ranks
        inside = r < tail_ranks
        tail += np.bincount(r[inside], w[inside], tail_ranks).astype(np.uint64)      # (exact: the sums stay below 2^53)
    return {"obs_rank": obs.astype(np.uint32), "labels": L, "perm_min": least, "tail": tail}


class Case:
    def __init__(self, masks, mults, N, table, n_ranks, tail_ranks, P, seed):
        self.N, self.W, self.F, self.P, self.T = N, words_for(N), len(masks), P, tail_ranks
        self.args = (masks, mults, N, case_words(N), table, n_ranks, tail_ranks, P, seed)
        self.inputs = [nat.DeviceBuffer.from_host(np.ascontiguousarray(a, dt).reshape(-1)) for a, dt in ((masks, np.uint64), (mults, np.uint32), (table, np.uint32))]
        self.outs = [nat.DeviceBuffer(max(self.F, 1) * 4), nat.DeviceBuffer(max(P, 1) * 8 * self.W), nat.DeviceBuffer(max(P, 1) * 4),
                     nat.DeviceBuffer(max(tail_ranks, 1) * 8)]

    def launch(self):
        masks, mults, n, cw, table, n_ranks, tail_ranks, P, seed = self.args
        nat.assoc_permute_wide_device(n, cw, self.F, *self.inputs, n_ranks, tail_ranks, P, seed, *self.outs, None)

    def read(self):
        o = self.outs
        return {"obs_rank": o[0].to_host(np.uint32, self.F), "labels": o[1].to_host(np.uint64, self.P * self.W).reshape(self.P, self.W),
                "perm_min": o[2].to_host(np.uint32, self.P), "tail": o[3].to_host(np.uint64, self.T)}

    def free(self):
        for b in self.inputs + self.outs:
            b.free()


def measure(case, repeats, host_entry=True):
    ms, ms_all = timed(case.launch, repeats)
    got = case.read()
    r = {"samples": case.N, "words": case.W, "features": case.F, "permutations": case.P, "pairs": case.F * case.P, "tail_ranks": case.T,
         "device_ms": ms, "device_ms_min": min(ms_all), "device_ms_max": max(ms_all), "device_ms_all": ms_all,
         "pairs_per_ns": round(case.F * case.P / (ms * 1e6), 2) if ms else None, "tail_total": int(got["tail"].sum(dtype=object)),
         "min_perm_rank": int(got["perm_min"].min())}
    if host_entry:
        t0 = time.perf_counter()
        host = nat.assoc_permute_wide(*case.args)
        r["host_entry_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        r["host_entry_same"] = bool(all(np.array_equal(host[k], got[k]) for k in got))
    return r, got


def shape_of(text):
    return tuple(int(x) for x in text.split("x")) if text else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=str, default="128,256,640,1024")
    ap.add_argument("--features", type=str, default="100000,1000000")
    ap.add_argument("--permutations", type=str, default="1000,10000")
    ap.add_argument("--max-p", dest="max_p", type=str, default="0.05")
    ap.add_argument("--dense", type=str, default="100000x10000x640")
    ap.add_argument("--shuffled", type=str, default="100000x10000x640")
    ap.add_argument("--numpy-shape", dest="numpy_shape", type=str, default="2000x200x130")
    ap.add_argument("--narrow", type=str, default="1000000x10000", help="features x permutations of the yardstick at 64 samples")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    max_p = asc.parse_max_p(a.max_p)
    if max_p is None or a.repeats < 1:
        raise SystemExit("--max-p is a decimal or a fraction 0 .. 1, --repeats 1 or more")
    samples = [int(x) for x in a.samples.split(",") if x]
    features, perms = [int(x) for x in a.features.split(",") if x], [int(x) for x in a.permutations.split(",") if x]
    if a.dry:
        masks, mults = seeded_rows(samples[0], min(features[0], 5000), a.seed)
        m = asc.popcount_rows(masks)
        print(json.dumps({"dry": True, "samples": samples, "features": features, "permutations": perms, "first_patterns": len(masks),
                          "ascending": bool((np.diff(m) >= 0).all()), "share_in_2_to_4_samples": round(float(((m >= 2) & (m <= 4)).mean()), 3)}))
        return
    res = {"device": nat.device_name(), "alternative": "greater", "max_p": a.max_p, "repeats": a.repeats, "seed": a.seed,
           "patterns": "tools/bench_assoc_wide.py seeded_rows: distinct rows, 99 in 100 in 2 to 4 samples, 1 % dense, ascending popcount; "
                       "multiplicity geometric(0.3); every other sample a case", "tables": {}, "shapes": {}}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    tables = {}

    def table_of(N):
        if N not in tables:
            t0 = time.perf_counter()
            table, p_of_rank = asc.rank_table_sums(N, (N + 1) // 2, "greater")
            tables[N] = (table, len(p_of_rank), sum(p <= max_p for p in p_of_rank))
            res["tables"][str(N)] = {"n_ranks": tables[N][1], "tail_ranks": tables[N][2], "build_s": round(time.perf_counter() - t0, 2)}
        return tables[N]

    def note(name, r):
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
    small = shape_of(a.numpy_shape)
    if small:
        F, P, N = small
        masks, mults = seeded_rows(N, F, a.seed)
        case = Case(masks, mults, N, *table_of(N), P, a.seed)
        r, got = measure(case, a.repeats)
        t0 = time.perf_counter()
        want = numpy_permute_wide(*case.args)
        r["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["same_as_numpy"] = bool(all(np.array_equal(np.asarray(want[k]).astype(got[k].dtype), got[k]) for k in got))
        res["numpy_shape"] = r
        note("numpy shape", r)
        case.free()
    narrow = shape_of(a.narrow)
    if narrow:      # the first yardstick: both entries at 64 samples on the same masks
        import bench_assoc
        F, P = narrow
        masks, mults = bench_assoc.seeded_patterns(F, a.seed)
        order = np.argsort(np.bitwise_count(masks), kind="stable")
        masks, mults = masks[order], mults[order]
        table16, p_of_rank = asc.rank_table(64, 32, "greater")
        n_ranks, tail_ranks = len(p_of_rank), sum(p <= max_p for p in p_of_rank)
        old = bench_assoc.Case(masks, mults, table16, n_ranks, tail_ranks, P, a.seed)
        ms, ms_all = timed(old.launch, a.repeats)
        got_old = old.read()
        old.free()
        case = Case(masks.reshape(-1, 1), mults, 64, table16.astype(np.uint32), n_ranks, tail_ranks, P, a.seed)
        case.args = case.args[:3] + (np.array([bench_assoc.CASES], np.uint64),) + case.args[4:]
        r, got = measure(case, a.repeats, host_entry=False)
        r.update({"narrow_device_ms": ms, "narrow_device_ms_min": min(ms_all), "narrow_device_ms_max": max(ms_all), "narrow_device_ms_all": ms_all,
                  "same_as_narrow": bool(all(np.array_equal(got_old[k].reshape(-1), got[k].reshape(-1)) for k in got))})
        res["narrow_yardstick"] = r
        note("64 samples, narrow beside wide", r)
        case.free()
    for N in samples:
        for F in features:
            masks, mults = seeded_rows(N, F, a.seed)
            for P in perms:
                case = Case(masks, mults, N, *table_of(N), P, a.seed)
                r, _ = measure(case, a.repeats)
                res["shapes"][f"{N}:{F}x{P}"] = r
                note(f"N {N}, {F}x{P}", r)
                case.free()
    shuffled = shape_of(a.shuffled)
    if shuffled:
        F, P, N = shuffled
        masks, mults = seeded_rows(N, F, a.seed)
        order = np.random.default_rng(a.seed).permutation(F)
        both = {}
        for name, (mk, ml) in (("ascending", (masks, mults)), ("shuffled", (masks[order], mults[order]))):
            case = Case(np.ascontiguousarray(mk), ml, N, *table_of(N), P, a.seed)
            both[name], got = measure(case, a.repeats, host_entry=False)
            both[name]["tail"], both[name]["least"] = got["tail"], got["perm_min"]
            case.free()
        same = bool(np.array_equal(both["ascending"].pop("tail"), both["shuffled"].pop("tail")) and
                    np.array_equal(both["ascending"].pop("least"), both["shuffled"].pop("least")))
        res["order"] = dict(both, same_null=same)
        note("ascending", both["ascending"])
        note("shuffled", both["shuffled"])
    dense = shape_of(a.dense)
    if dense:
        F, P, N = dense
        table, n_ranks, _ = table_of(N)
        row = np.zeros(words_for(N), np.uint64)
        row[:] = 0x00000000FFFF00FF      # one pattern everywhere, every rank in the tail: each pair is an LDS add
        row[-1] &= np.uint64((1 << (N - 64 * (len(row) - 1))) - 1 if N % 64 else (1 << 64) - 1)
        case = Case(np.tile(row, (F, 1)), np.ones(F, np.uint32), N, table, n_ranks, n_ranks, P, a.seed)
        r, got = measure(case, a.repeats, host_entry=False)
        r["every_pair_counted"] = bool(r["tail_total"] == F * P)
        res["dense"] = r
        note("dense", r)
        case.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
