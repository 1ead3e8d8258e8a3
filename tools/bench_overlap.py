#!/usr/bin/env python3
"""The overlap step (`overlap`) on the GPU: one JSON line with, for seeded tables of 8 samples x 10^5 and 10^6 rows (strings of
11 to 18 random residues under 60 classes, Zipf-like weights; three in ten of a sample's rows are drawn from a pool the
samples share, so that about a tenth of the groups are public):
  - the host entry dcrx_overlap_run with everything it exports, as the stage calls it (wall clock, with its copies in and
    out), median of --repeats after a warm-up;
  - the primitive dcrx_overlap_pairs_device on device buffers holding the same tables' cells (device events around its two
    launches, median of --repeats after a warm-up); its planes are compared with the run's: they must agree;
  - the baseline there is, up to --baseline-up-to rows: the test util's Python dict on one thread
    (tests/overlap_util.expected_overlap) on the same table; the two sides' statistics and planes are compared.
There is no pass mark.
Usage: tools/bench_overlap.py [--samples 8] [--rows 100000,1000000] [--repeats 5] [--baseline-up-to 800000] [--no-baseline]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402
from tests import overlap_util as ou  # noqa: E402

SHARED_FRACTION = 0.3      # of a sample's rows; the pool holds twice that many keys, so a sample draws every other one


def seeded_tables(S, n, seed):
    """(samples, classes, off, text, weights) of S samples x n rows."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(ou.AMINO.encode(), np.uint8)
    width = 18
    n_shared = int(n * SHARED_FRACTION)
    pool = 2 * n_shared
    n_keys = pool + S * (n - n_shared)
    ids = []
    for a in range(S):
        own = pool + a * (n - n_shared) + np.arange(n - n_shared)
        row_ids = np.concatenate([rng.choice(pool, n_shared, replace=False), own])
        rng.shuffle(row_ids)
        ids.append(row_ids)
    ids = np.concatenate(ids)
    key_len = rng.integers(11, width + 1, n_keys)
    key_mat = letters[rng.integers(0, len(letters), (n_keys, width))]
    key_class = rng.integers(0, 60, n_keys).astype(np.uint32)
    lens = key_len[ids]
    off = np.zeros(len(ids) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    text = key_mat[ids][np.arange(width)[None, :] < lens[:, None]].tobytes()
    weights = np.maximum(1, (1000 / (1 + rng.pareto(1.2, len(ids)) * 20)).astype(np.uint64))
    return np.repeat(np.arange(S, dtype=np.uint32), n), key_class[ids], off, text, weights


def time_run(samples, classes, off, text, weights, S, repeats):
    wall = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        result, stats = nat.overlap(samples, classes, off, text, weights, S, 2)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    return result, stats, {"overlap_run_ms": round(statistics.median(wall), 2), "overlap_run_ms_all": [round(x, 2) for x in wall]}


def time_pairs(result, samples, weights, S, repeats):
    """The primitive on the table's cells, made here with numpy out of group_of."""
    key = result["group_of"].astype(np.uint64) * 64 + samples
    cells, inverse = np.unique(key, return_inverse=True)
    cell_weight = np.bincount(inverse, weights=weights.astype(np.float64)).astype(np.uint32)      # (sums far below 2^53)
    n_groups = int(result["group_of"].max()) + 1
    cell_off = np.zeros(n_groups + 1, np.uint32)
    cell_off[1:] = np.cumsum(np.bincount((cells >> 6).astype(np.int64), minlength=n_groups))
    bufs = [nat.DeviceBuffer.from_host(a) for a in (cell_off, (cells & 63).astype(np.uint32), cell_weight)]
    d_planes = nat.DeviceBuffer(5 * S * S * 8)
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        nat.check(nat.lib().dcrx_memset_device(d_planes.ptr, 0, 5 * S * S * 8))
        e0.record()
        nat.overlap_pairs_device(n_groups, bufs[0], bufs[1], bufs[2], S, d_planes)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    planes = d_planes.to_host(np.uint64, 5 * S * S).reshape(5, S, S)
    same = all(np.array_equal(planes[p], result[name]) for p, name in enumerate(nat.OVERLAP_PLANES))
    for b in bufs + [d_planes]:
        b.free()
    return {"pairs_device_ms": round(statistics.median(ms), 3), "pairs_device_ms_all": [round(x, 3) for x in ms], "cells": int(len(cells)),
            "groups": n_groups, "pairs_planes_equal_the_runs": bool(same)}


def time_baseline(samples, classes, off, text, weights, S, result, stats):
    strings = ou.row_strings(off, text)
    t0 = time.perf_counter()
    want, wstats = ou.expected_overlap(samples, classes, strings, weights, S, 2)
    ms = (time.perf_counter() - t0) * 1e3
    same = wstats == stats and all([int(x) for x in want[k].reshape(-1)] == [int(x) for x in result[k].reshape(-1)]
                                   for k in nat.OVERLAP_PLANES)
    return {"python_dict_ms": round(ms, 1), "same_statistics_and_planes": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--rows", type=str, default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-up-to", type=int, default=800_000, help="total rows up to which the Python baseline runs")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    S = a.samples
    res = {"device": nat.device_name(), "table": f"{S} samples, 11-18 residues, 60 classes, {SHARED_FRACTION} of a sample's rows from a "
           "shared pool of twice that size, seed = rows", "repeats": a.repeats, "tables": {}}
    for n in (int(x) for x in a.rows.split(",")):
        samples, classes, off, text, weights = seeded_tables(S, n, seed=n)
        result, stats, r = time_run(samples, classes, off, text, weights, S, a.repeats)
        r = dict({"samples": S, "rows_per_sample": n, "rows": S * n, "text_bytes": len(text)}, **r)
        r["stats"] = stats
        r["public_fraction_of_groups"] = round(stats["shared_groups"] / max(1, stats["groups"]), 4)
        r.update(time_pairs(result, samples, weights, S, a.repeats))
        if not a.no_baseline and S * n <= a.baseline_up_to:
            r["baseline"] = time_baseline(samples, classes, off, text, weights, S, result, stats)
        elif not a.no_baseline:
            r["baseline"] = f"not measured: more than --baseline-up-to {a.baseline_up_to} rows"
        res["tables"][f"{S}x{n}"] = r
        print(f"{S}x{n}: run {r['overlap_run_ms']} ms, pairs {r['pairs_device_ms']} ms", file=sys.stderr, flush=True)      # (progress)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
