#!/usr/bin/env python3
"""The permutation null on the GPU (include/dcrx.h "association"): one JSON line with, for seeded presence patterns of N = 64
samples, 32 of them cases — most features in 2 to 4 samples, one in a hundred dense, all patterns distinct, a multiplicity of 1
and more each — and the table of the one-sided exact test (`greater`) with the ranks at or below --max-p as the tail:
  - dcrx_assoc_permute_device (the labels kernel and the permute kernel) under device events: the median of --repeats after a
    warm-up, with the smallest and the largest, and the pairs a nanosecond;
  - dcrx_assoc_permute, the host entry, by the wall clock (the allocation, the uploads and the copies back included);
  - beside both, at --numpy-shape (10^4 features, 10^3 permutations), the numpy form of the contract
    (tests/assoc_util.expected_permute) on one thread, which the device's four arrays must equal;
  - a dense case, which prices the LDS adds: ONE pattern everywhere and tail_ranks = n_ranks, so every (feature, relabeling) pair
    adds to a tail cell.
--out FILE rewrites the result so far after every shape.  --dry checks the arguments and builds the first patterns, and touches
no device.
Usage: tools/bench_assoc.py [--features 100000,1000000] [--permutations 1000,10000] [--max-p 0.05] [--dense 100000x10000]
                            [--numpy-shape 10000x1000] [--repeats 15] [--seed 1] [--dry] [--out FILE]"""
import argparse
import itertools
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

N, N1 = 64, 32
CASES = 0x5555555555555555      # every other sample


def seeded_patterns(F, seed):
    """F distinct presence patterns of 64 samples and their multiplicities: 3 in 10 draws each in 2, 3 and 4 samples, the tenth
    in 5 to 16 (samples drawn with replacement, so a few fall below; 64 samples have only 2 016 patterns of 2 and 41 664 of 3, so
    among many DISTINCT patterns those of 4 and more take their place), one in a hundred a pattern of 64 fair bits."""
    rng = np.random.default_rng(seed)
    have = np.zeros(0, np.uint64)
    while len(have) < F:
        n = F - len(have) + 1024
        m = np.where(rng.integers(0, 10, n) < 9, rng.integers(2, 5, n), np.minimum(4 + rng.geometric(0.5, n), 16))
        where = rng.integers(0, N, size=(n, 16)).astype(np.uint64)
        bits = np.where(np.arange(16)[None, :] < m[:, None], np.uint64(1) << where, np.uint64(0))
        masks = np.bitwise_or.reduce(bits, axis=1)
        dense = rng.integers(0, 100, n) == 0
        masks[dense] = rng.integers(0, 1 << 63, int(dense.sum()), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, int(dense.sum()), dtype=np.uint64)
        have = np.unique(np.concatenate([have, masks]))
    have = rng.permutation(have)[:F]
    return np.ascontiguousarray(have), rng.geometric(0.3, F).astype(np.uint32)


class Case:
    def __init__(self, masks, mults, table, n_ranks, tail_ranks, P, seed):
        self.args = (masks, mults, N, CASES, table, n_ranks, tail_ranks, P, seed)
        self.F, self.P, self.T = len(masks), P, tail_ranks
        self.inputs = [nat.DeviceBuffer.from_host(np.ascontiguousarray(a, dt)) for a, dt in ((masks, np.uint64), (mults, np.uint32), (table, np.uint16))]
        self.outs = [nat.DeviceBuffer(max(self.F, 1) * 4), nat.DeviceBuffer(max(P, 1) * 8), nat.DeviceBuffer(max(P, 1) * 4),
                     nat.DeviceBuffer(max(tail_ranks, 1) * 8)]

    def launch(self):
        masks, mults, n, c, table, n_ranks, tail_ranks, P, seed = self.args
        nat.assoc_permute_device(n, c, self.F, *self.inputs, n_ranks, tail_ranks, P, seed, *self.outs, None)

    def read(self):
        o = self.outs
        return {"obs_rank": o[0].to_host(np.uint32, self.F), "labels": o[1].to_host(np.uint64, self.P), "perm_min": o[2].to_host(np.uint32, self.P),
                "tail": o[3].to_host(np.uint64, self.T)}

    def free(self):
        for b in self.inputs + self.outs:
            b.free()


def measure(case, repeats):
    ms, ms_all = timed(case.launch, repeats)
    got = case.read()
    r = {"features": case.F, "permutations": case.P, "pairs": case.F * case.P, "tail_ranks": case.T, "device_ms": ms, "device_ms_min": min(ms_all),
         "device_ms_max": max(ms_all), "device_ms_all": ms_all, "pairs_per_ns": round(case.F * case.P / (ms * 1e6), 2) if ms else None,
         "tail_total": int(got["tail"].sum(dtype=object)), "min_perm_rank": int(got["perm_min"].min())}
    t0 = time.perf_counter()
    host = nat.assoc_permute(*case.args)
    r["host_entry_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    r["host_entry_same"] = bool(all(np.array_equal(host[k], got[k]) for k in got))
    return r, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=str, default="100000,1000000")
    ap.add_argument("--permutations", type=str, default="1000,10000")
    ap.add_argument("--max-p", dest="max_p", type=str, default="0.05")
    ap.add_argument("--dense", type=str, default="100000x10000")
    ap.add_argument("--numpy-shape", dest="numpy_shape", type=str, default="10000x1000")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    max_p = asc.parse_max_p(a.max_p)
    if max_p is None or a.repeats < 1:
        raise SystemExit("--max-p is a decimal or a fraction 0 .. 1, --repeats 1 or more")
    shapes = list(itertools.product((int(x) for x in a.features.split(",")), (int(x) for x in a.permutations.split(","))))
    dense = tuple(int(x) for x in a.dense.split("x")) if a.dense else None
    small = tuple(int(x) for x in a.numpy_shape.split("x")) if a.numpy_shape else None
    table, p_of_rank = asc.rank_table(N, N1, "greater")
    n_ranks, tail_ranks = len(p_of_rank), sum(p <= max_p for p in p_of_rank)
    if a.dry:
        masks, mults = seeded_patterns(min(shapes[0][0], 5000), a.seed)
        m = np.bitwise_count(masks)
        print(json.dumps({"dry": True, "shapes": [f"{f}x{p}" for f, p in shapes], "dense": dense, "numpy_shape": small, "n_ranks": n_ranks,
                          "tail_ranks": tail_ranks, "first_patterns": len(masks), "share_in_2_to_4_samples": round(float(((m >= 2) & (m <= 4)).mean()), 3)}))
        return
    res = {"device": nat.device_name(), "samples": N, "cases": N1, "alternative": "greater", "max_p": a.max_p, "n_ranks": n_ranks,
           "tail_ranks": tail_ranks, "repeats": a.repeats, "seed": a.seed,
           "patterns": "tools/bench_assoc.py seeded_patterns: distinct masks, 9 draws in 10 in 2 to 4 samples, the rest in 5 to 16, 1 % dense; multiplicity geometric(0.3)",
           "shapes": {}}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    if small:
        from tests import assoc_util as au
        masks, mults = seeded_patterns(small[0], a.seed)
        case = Case(masks, mults, table, n_ranks, tail_ranks, small[1], a.seed)
        r, got = measure(case, a.repeats)
        t0 = time.perf_counter()
        want = au.expected_permute(*case.args)
        r["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["same_as_numpy"] = bool(all(np.array_equal(np.asarray(want[k]).astype(got[k].dtype), got[k]) for k in got))
        res["numpy_shape"] = r
        print("numpy shape: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
        case.free()
    for F in sorted({f for f, _ in shapes}):
        masks, mults = seeded_patterns(F, a.seed)
        m = np.bitwise_count(masks)
        for P in [p for f, p in shapes if f == F]:
            case = Case(masks, mults, table, n_ranks, tail_ranks, P, a.seed)
            r, _ = measure(case, a.repeats)
            r["share_in_2_to_4_samples"] = round(float(((m >= 2) & (m <= 4)).mean()), 3)
            res["shapes"][f"{F}x{P}"] = r
            print(f"{F}x{P}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
            save()
            case.free()
    if dense:
        F, P = dense
        # one pattern everywhere, every rank in the tail: each pair is an LDS add, and a wave's lanes share a few cells
        case = Case(np.full(F, 0x00000000FFFF00FF, np.uint64), np.ones(F, np.uint32), table, n_ranks, n_ranks, P, a.seed)
        r, got = measure(case, a.repeats)
        r["every_pair_counted"] = bool(r["tail_total"] == F * P)
        res["dense"] = r
        print("dense: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
        case.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
