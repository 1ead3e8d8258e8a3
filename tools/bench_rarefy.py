#!/usr/bin/env python3
"""The downsampling step (`overlap --downsample`) on the GPU: one JSON line with, for seeded tables of 8 samples x 10^6 rows
holding 10^7 and 10^8 reads in all (every row one read at least, the rest spread Zipf-like, and a sample's top row holding 15 %
of its reads), downsampled to half of the smallest sample:
  - the primitive dcrx_downsample_device on device buffers (device events around the call, median of --repeats after a
    warm-up); its outputs are compared with the host entry's: they must agree;
  - the host entry dcrx_downsample, as the stage calls it (wall clock, with its copies in and out), median of --repeats after a
    warm-up;
  - the baseline there is, up to --baseline-up-to reads: the test util's numpy brute force on one thread
    (tests/rarefy_util.expected_downsample: every key, sorted) on the same table; the four outputs are compared.
There is no pass mark.
Usage: tools/bench_rarefy.py [--samples 8] [--rows 1000000] [--reads 10000000,100000000] [--repeats 5] [--baseline-up-to 100000000]
       [--no-baseline]"""
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
from tests import rarefy_util as ru  # noqa: E402

TOP_FRACTION = 0.15


def seeded_table(S, rows, reads, seed):
    """(samples, weights) of S samples x rows rows with about reads / S reads each (unequal: sample a holds 1 + a / (4 S) shares)."""
    rng = np.random.default_rng(seed)
    share = np.array([1 + a / (4 * S) for a in range(S)])
    weights = []
    for a in range(S):
        X = int(reads * share[a] / share.sum())
        top = int(X * TOP_FRACTION)
        p = 1 / (1 + rng.pareto(1.2, rows - 1) * 20)
        w = 1 + rng.multinomial(max(0, X - top - (rows - 1)), p / p.sum()).astype(np.uint64)
        weights.append(np.insert(w, rows // 3, top))
    return np.repeat(np.arange(S, dtype=np.uint32), rows), np.concatenate(weights)


def time_device(samples, weights, S, depths, seed, repeats):
    m = len(samples)
    work = nat.downsample_work_bytes(m, S)
    bufs = [nat.DeviceBuffer.from_host(a) for a in (samples, weights, depths)]
    outs = [nat.DeviceBuffer(8 * n) for n in (m, S, S, S)]
    d_work = nat.DeviceBuffer(work)
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        nat.downsample_device(S, m, *bufs, seed, *outs, d_work, work)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    got = {name: b.to_host(np.uint64, n) for name, b, n in zip(ru.OUTPUTS, outs, (m, S, S, S))}
    for b in bufs + outs + [d_work]:
        b.free()
    return got, {"downsample_device_ms": round(statistics.median(ms), 3), "downsample_device_ms_all": [round(x, 3) for x in ms],
                 "work_bytes": work}


def time_host_entry(samples, weights, S, depths, seed, repeats):
    wall = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        got = nat.downsample(samples, weights, S, depths, seed)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    return got, {"downsample_ms": round(statistics.median(wall), 2), "downsample_ms_all": [round(x, 2) for x in wall]}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ru.OUTPUTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reads", type=str, default="10000000,100000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-up-to", type=int, default=100_000_000, help="total reads up to which the numpy baseline runs")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    S = a.samples
    res = {"device": nat.device_name(), "table": f"{S} samples x {a.rows} rows, a sample's top row {TOP_FRACTION} of its reads, depth = half the "
           "smallest sample, seed = reads", "repeats": a.repeats, "tables": {}}
    for reads in (int(x) for x in a.reads.split(",")):
        samples, weights = seeded_table(S, a.rows, reads, seed=reads)
        per_sample = np.bincount(samples, weights=weights.astype(np.float64)).astype(np.uint64)      # (sums far below 2^53)
        depths = np.full(S, int(per_sample.min()) // 2, np.uint64)
        dev, r = time_device(samples, weights, S, depths, 1, a.repeats)
        host, h = time_host_entry(samples, weights, S, depths, 1, a.repeats)
        r.update(h)
        r = dict({"samples": S, "rows": len(samples), "reads": int(weights.sum()), "depth": int(depths[0]),
                  "top_row_fraction": round(float(weights.max()) / float(per_sample[samples[int(weights.argmax())]]), 4),
                  "reads_per_ms_device": round(float(weights.sum()) / r["downsample_device_ms"])}, **r)
        r["device_equals_host_entry"] = bool(same(dev, host))
        r["kept_adds_up"] = bool(np.array_equal(np.bincount(samples, weights=host["kept"].astype(np.float64)).astype(np.uint64), host["depth_used"]))
        if not a.no_baseline and reads <= a.baseline_up_to:
            t0 = time.perf_counter()
            want = ru.expected_downsample(samples, weights, S, depths, 1)
            r["baseline"] = {"numpy_brute_force_ms": round((time.perf_counter() - t0) * 1e3, 1), "same_outputs": bool(same(host, want))}
        elif not a.no_baseline:
            r["baseline"] = f"not measured: more than --baseline-up-to {a.baseline_up_to} reads"
        res["tables"][f"{S}x{a.rows}_{reads}"] = r
        print(f"{reads} reads: device {r['downsample_device_ms']} ms, host entry {r['downsample_ms']} ms", file=sys.stderr, flush=True)      # (progress)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
