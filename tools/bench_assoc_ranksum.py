#!/usr/bin/env python3
"""The rank-sum null on the GPU (include/dcrx.h "association, rank-sum"): one JSON line, also written to --out, with, for N = 64
samples, 32 of them cases, alternative `greater` and the (up to 1024) largest distinct observed scores as the edges:
  - dcrx_assoc_ranksum_device (prepare, labels and permute kernels) under device events around the whole call: the median of
    --repeats after a warm-up, with the smallest and the largest, on seeded sparse features — 99 in 100 non-zero in 2 to 4
    samples, one in a hundred in all of them — at every --shapes entry;
  - BESIDE it dcrx_assoc_permute_device on the presence patterns of the same features with the one-sided exact test's table and
    the ranks at or below 0.05 as the tail: the presence null on the same shape, the yardstick for what seven planes cost;
  - a dense case: every feature distinct values in all 64 samples;
  - a case with edges = [0]: every pair takes the tail branch;
  - at --numpy-shape the numpy form of the contract (tests/assoc_ranksum_util.expected_ranksum) on one thread, which the
    device's five arrays must equal.
--dry checks the arguments and builds the first features, and touches no device.
Usage: tools/bench_assoc_ranksum.py [--shapes 10000x1000,100000x10000,1000000x10000] [--dense 100000x10000] [--all-tail 100000x10000]
                                    [--numpy-shape 10000x1000] [--repeats 15] [--seed 1] [--dry] [--out FILE]"""
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

N, N1 = 64, 32
CASES = 0x5555555555555555      # every other sample
DEFAULT_OUT = os.path.join(ROOT, "profiles", "assoc_ranksum", "bench_assoc_ranksum.json")


def seeded_values(F, seed, dense=False):
    """F features x 64 samples of values: 99 in 100 non-zero in 2 to 4 samples (values 1 .. 9), one in a hundred non-zero in all
    with ties; dense: every feature 64 distinct values."""
    rng = np.random.default_rng(seed)
    if dense:
        return np.argsort(rng.random((F, N)), axis=1).astype(np.int64) + 1
    x = np.zeros((F, N), dtype=np.int64)
    m = rng.integers(2, 5, F)
    where = np.argsort(rng.random((F, N)), axis=1)[:, :4]
    for j in range(4):
        rows = np.flatnonzero(m > j)
        x[rows, where[rows, j]] = rng.integers(1, 10, len(rows))
    full = np.flatnonzero(rng.integers(0, 100, F) == 0)
    x[full] = rng.integers(1, 40, size=(len(full), N))
    return x


def inputs(x):
    a = asc.rank_scores(x, range(N), 1)
    planes, off, sc = asc.ranksum_inputs(a, N1)
    D = asc.ranksum_D(a, CASES, N1)
    obs = (np.clip(D, 0, (1 << nat.ASSOC_RANKSUM_SHIFT) - 1) * sc.astype(np.int64)) >> nat.ASSOC_RANKSUM_SHIFT      # greater
    return planes, off, sc, obs


class Ranksum:
    def __init__(self, planes, off, sc, mults, edges, P, seed):
        self.args = (planes, off, sc, mults, N, CASES, 0, edges, P, seed)
        self.F, self.P, self.E = len(planes), P, len(edges)
        self.inputs = [nat.DeviceBuffer.from_host(np.ascontiguousarray(a, dt).reshape(-1))
                       for a, dt in ((planes, np.uint64), (off, np.uint32), (sc, np.uint32), (mults, np.uint32), (edges, np.uint32))]
        self.outs = [nat.DeviceBuffer(self.F * 4), nat.DeviceBuffer(P * 8), nat.DeviceBuffer(P * 4), nat.DeviceBuffer(self.F * 4), nat.DeviceBuffer(self.E * 8)]

    def launch(self):
        i, o = self.inputs, self.outs
        nat.assoc_ranksum_device(N, CASES, 0, self.F, i[0], i[1], i[2], i[3], self.E, i[4], self.P, self.args[9], o[0], o[1], o[2], o[3], o[4], None)

    def read(self):
        o = self.outs
        return {"obs_score": o[0].to_host(np.uint32, self.F), "labels": o[1].to_host(np.uint64, self.P), "perm_max": o[2].to_host(np.uint32, self.P),
                "exceed": o[3].to_host(np.uint32, self.F), "tail": o[4].to_host(np.uint64, self.E)}

    def free(self):
        for b in self.inputs + self.outs:
            b.free()


def measure(case, repeats):
    ms, ms_all = timed(case.launch, repeats)
    got = case.read()
    pairs = case.F * case.P
    return {"features": case.F, "permutations": case.P, "pairs": pairs, "edges": case.E, "device_ms": ms, "device_ms_min": min(ms_all),
            "device_ms_max": max(ms_all), "device_ms_all": ms_all, "pairs_per_ns": round(pairs / (ms * 1e6), 2) if ms else None,
            "tail_total": int(got["tail"].sum(dtype=object)), "max_perm_score": int(got["perm_max"].max())}, got


def presence_beside(x, mults, P, seed, repeats, table, n_ranks, tail_ranks):
    """dcrx_assoc_permute_device on the presence patterns of the same features."""
    masks = asc.presence_masks(x, range(N), 1)
    ins = [nat.DeviceBuffer.from_host(np.ascontiguousarray(a, dt)) for a, dt in ((masks, np.uint64), (mults, np.uint32), (table, np.uint16))]
    outs = [nat.DeviceBuffer(len(masks) * 4), nat.DeviceBuffer(P * 8), nat.DeviceBuffer(P * 4), nat.DeviceBuffer(max(tail_ranks, 1) * 8)]
    ms, ms_all = timed(lambda: nat.assoc_permute_device(N, CASES, len(masks), *ins, n_ranks, tail_ranks, P, seed, *outs, None), repeats)
    for b in ins + outs:
        b.free()
    return {"device_ms": ms, "device_ms_min": min(ms_all), "device_ms_max": max(ms_all), "device_ms_all": ms_all, "tail_ranks": tail_ranks}


def shape_of(text):
    f, p = text.split("x")
    return int(f), int(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="10000x1000,100000x10000,1000000x10000")
    ap.add_argument("--dense", type=str, default="100000x10000")
    ap.add_argument("--all-tail", dest="all_tail", type=str, default="100000x10000")
    ap.add_argument("--numpy-shape", dest="numpy_shape", type=str, default="10000x1000")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", type=str, default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.repeats < 1:
        raise SystemExit("--repeats is 1 or more")
    shapes = [shape_of(w) for w in a.shapes.split(",") if w]
    dense, all_tail, small = (shape_of(w) if w else None for w in (a.dense, a.all_tail, a.numpy_shape))
    if a.dry:
        x = seeded_values(min(shapes[0][0], 5000), a.seed)
        nz = (x > 0).sum(axis=1)
        planes, off, sc, obs = inputs(x)
        print(json.dumps({"dry": True, "shapes": shapes, "dense": dense, "all_tail": all_tail, "numpy_shape": small, "first_features": len(x),
                          "share_in_2_to_4_samples": round(float(((nz >= 2) & (nz <= 4)).mean()), 3), "distinct_scores": int(len(np.unique(obs)))}))
        return
    table, p_of_rank = asc.rank_table(N, N1, "greater")
    n_ranks, tail_ranks = len(p_of_rank), sum(p <= asc.parse_max_p("0.05") for p in p_of_rank)
    res = {"device": nat.device_name(), "samples": N, "cases": N1, "alternative": "greater", "repeats": a.repeats, "seed": a.seed,
           "features_are": "tools/bench_assoc_ranksum.py seeded_values: 99 in 100 non-zero in 2 to 4 samples, 1 in 100 in all 64; multiplicity 1",
           "timed": "device events around the whole device call (prepare, labels, permute): median, smallest, largest of the repeats after a warm-up",
           "shapes": {}}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    def edges_of(obs):
        return np.unique(obs)[-nat.ASSOC_RANKSUM_MAX_EDGES:].astype(np.uint32)
    if small:
        from tests import assoc_ranksum_util as ru
        x = seeded_values(small[0], a.seed)
        planes, off, sc, obs = inputs(x)
        case = Ranksum(planes, off, sc, np.ones(len(x), np.uint32), edges_of(obs), small[1], a.seed)
        r, got = measure(case, a.repeats)
        t0 = time.perf_counter()
        want = ru.expected_ranksum(*case.args)
        r["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["same_as_numpy"] = bool(all(np.array_equal(np.asarray(want[k]).astype(got[k].dtype), got[k]) for k in got))
        r["host_observed_same"] = bool(np.array_equal(obs, got["obs_score"].astype(np.int64)))
        res["numpy_shape"] = r
        print("numpy shape: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
        case.free()
    for F in sorted({f for f, _ in shapes}):
        x = seeded_values(F, a.seed)
        planes, off, sc, obs = inputs(x)
        mults = np.ones(F, np.uint32)
        zero_planes = float((planes == 0).mean())
        for P in [p for f, p in shapes if f == F]:
            case = Ranksum(planes, off, sc, mults, edges_of(obs), P, a.seed)
            r, _ = measure(case, a.repeats)
            case.free()
            r["share_of_zero_planes"] = round(zero_planes, 3)
            r["presence_null_beside"] = presence_beside(x, mults, P, a.seed, a.repeats, table, n_ranks, tail_ranks)
            r["ranksum_over_presence"] = round(r["device_ms"] / r["presence_null_beside"]["device_ms"], 2) if r["presence_null_beside"]["device_ms"] else None
            res["shapes"][f"{F}x{P}"] = r
            print(f"{F}x{P}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
            save()
    for name, shape, kind in (("dense", dense, "dense"), ("all_tail", all_tail, "sparse")):
        if not shape:
            continue
        x = seeded_values(shape[0], a.seed + 1, dense=kind == "dense")
        planes, off, sc, obs = inputs(x)
        edges = np.zeros(1, np.uint32) if name == "all_tail" else edges_of(obs)
        case = Ranksum(planes, off, sc, np.ones(shape[0], np.uint32), edges, shape[1], a.seed)
        r, got = measure(case, a.repeats)
        case.free()
        if name == "all_tail":
            r["every_pair_counted"] = bool(r["tail_total"] == shape[0] * shape[1])
        r["share_of_zero_planes"] = round(float((planes == 0).mean()), 3)
        res[name] = r
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
