#!/usr/bin/env python3
"""The CDR3 network (`--clonotypes --cdr3-network`) on the GPU: one JSON line with, for seeded tables of 10^5, 10^6 and
4 * 10^6 nodes (strings of 11 to 18 random residues, a fifth of the nodes planted one or two substitutions from another node
and in its class, Zipf-like weights in descending order), under class `none` and under 60 classes, at D = 1 and 2:
  - the primitive dcrx_cdr3_neighbours_device on device buffers with an adjacency of the exact size (device events, median of
    --repeats after a warm-up);
  - the host entry dcrx_cdr3_network without the edges, as the stage calls it (wall clock, with its copies in and out),
    median of --repeats after a warm-up;
  - at 10^5 nodes only, the baseline there is: the test util's masked-position search and union-find
    (tests/cdr3_network_util.expected_network) on one Python thread.
The two sides' edge and cluster counts are compared: they must agree.
--metrics hamming,levenshtein times both metrics on the same tables, their runs interleaved repeat by repeat (the default,
hamming alone, prints what it always printed); a Levenshtein entry is keyed "<nodes>/<classes>/D<d>/levenshtein", its baseline
is the symmetric-deletion search of tests/cdr3_lev_util.expected_lev_network, and a table whose walk — quadratic in the class —
is estimated from the same metric's figure at a smaller size to take more than --skip-above-s seconds is skipped and says so.
Usage: tools/bench_cdr3_network.py [--sizes 100000,1000000,4000000] [--repeats 5] [--no-baseline] [--classes none,60] [--distances 1,2]
                                   [--metrics hamming] [--skip-above-s 180]"""
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
from tests import cdr3_lev_util as clu  # noqa: E402
from tests import cdr3_network_util as cnu  # noqa: E402

BASELINE_AT = 100_000


def seeded_table(n, seed, n_classes):
    """(classes, aa_off, aa_text, weights) of n nodes; what it held goes into the result beside the times."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(cnu.AMINO.encode(), np.uint8)
    width = 18
    lens = rng.integers(11, width + 1, n)
    mat = letters[rng.integers(0, len(letters), (n, width))]
    classes = rng.integers(0, n_classes, n).astype(np.uint32) if n_classes > 1 else np.zeros(n, np.uint32)
    # a fifth of the nodes: a copy of another node with one or two positions drawn again, in that node's class
    planted = rng.choice(n, n // 5, replace=False)
    free = np.setdiff1d(np.arange(n), planted)
    src = free[rng.integers(0, len(free), len(planted))]
    mat[planted], lens[planted], classes[planted] = mat[src], lens[src], classes[src]
    for k in range(2):
        hit = planted if k == 0 else planted[rng.random(len(planted)) < 0.5]
        mat[hit, rng.integers(0, lens[hit])] = letters[rng.integers(0, len(letters), len(hit))]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    text = mat[np.arange(width)[None, :] < lens[:, None]].tobytes()
    weights = np.sort(np.maximum(1, (1000 / (1 + rng.pareto(1.2, n) * 20)).astype(np.uint64)))[::-1].copy()
    return classes, off, text, weights


def _metric_arg(metric):
    return None if metric == "hamming" else metric      # (hamming goes through the entries that have no metric)


def time_device(classes, off, text, D, repeats, metrics=("hamming",)):
    """Per metric the primitive's times; the metrics' runs are interleaved repeat by repeat."""
    m = len(classes)
    d_cls, d_off = nat.DeviceBuffer.from_host(classes), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb, d_work, need, d_adj, ms = {}, {}, {}, {}, {}
    for metric in metrics:
        wb[metric] = nat.cdr3net_work_bytes(m, len(text), metric=_metric_arg(metric))
        d_work[metric] = nat.DeviceBuffer(wb[metric])
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, None, 0, d_need, d_work[metric], wb[metric],
                                   metric=_metric_arg(metric))
        nat.check(nat.lib().dcrx_synchronize())
        need[metric] = int(d_need.to_host(np.uint64, 1)[0])
        d_adj[metric] = nat.DeviceBuffer(max(16, need[metric] * 4))
        ms[metric] = []
    e0, e1 = nat.Event(), nat.Event()
    for k in range(repeats + 1):
        for metric in metrics:
            e0.record()
            nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, d_adj[metric], need[metric], d_need,
                                       d_work[metric], wb[metric], metric=_metric_arg(metric))
            e1.record()
            e1.synchronize()
            if k:
                ms[metric].append(e0.elapsed_ms(e1))
    return {metric: {"neighbours_device_ms": round(statistics.median(ms[metric]), 3),
                     "neighbours_device_ms_all": [round(x, 3) for x in ms[metric]], "adjacency_entries": need[metric],
                     "work_bytes": wb[metric]} for metric in metrics}


def time_host_entry(classes, off, text, weights, D, repeats, metric="hamming"):
    wall = []
    more = {} if metric == "hamming" else {"metric": metric}
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        _, stats = nat.cdr3_network(classes, off, text, weights, D, **more)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"cdr3_network_ms": round(statistics.median(wall), 2), "cdr3_network_ms_all": [round(x, 2) for x in wall], "stats": stats}


def time_baseline(classes, off, text, weights, D, metric="hamming"):
    strings = cnu.node_strings(off, text)
    t0 = time.perf_counter()
    if metric == "hamming":
        _, stats = cnu.expected_network(classes, strings, weights, D)
        name = "python_masked_search_ms"
    else:
        _, stats = clu.expected_lev_network(classes, strings, weights, D)
        name = "python_symmetric_deletion_ms"
    return {name: round((time.perf_counter() - t0) * 1e3, 1), "edges": stats["edges"], "clusters": stats["clusters_out"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--classes", type=str, default="none,60")
    ap.add_argument("--distances", type=str, default="1,2")
    ap.add_argument("--metrics", type=str, default="hamming")
    ap.add_argument("--skip-above-s", type=float, default=180.0)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    metrics = a.metrics.split(",")
    for metric in metrics:
        nat.cdr3_metric_code(metric)
    res = {"device": nat.device_name(), "table": "11-18 residues, a fifth planted at 1-2 substitutions, seed = nodes", "repeats": a.repeats,
           "tables": {}}
    seen_ms = {}      # (classes, distance, metric) -> (nodes, the primitive's ms) of the largest table measured so far
    for n in (int(x) for x in a.sizes.split(",")):
        for cls in a.classes.split(","):
            classes, off, text, weights = seeded_table(n, seed=n, n_classes=1 if cls == "none" else int(cls))
            for D in (int(x) for x in a.distances.split(",")):
                run, skipped = [], {}
                for metric in metrics:
                    before = seen_ms.get((cls, D, metric))
                    estimate = before[1] * (n / before[0]) ** 2 * (2 * a.repeats + 4) / 1e3 if before and metric != "hamming" else 0.0
                    if estimate > a.skip_above_s:
                        skipped[metric] = f"skipped: about {estimate:.0f} s for its {2 * a.repeats + 4} walks, from {before[1]} ms at {before[0]} nodes"
                    else:
                        run.append(metric)
                dev = time_device(classes, off, text, D, a.repeats, run) if run else {}
                for metric in metrics:
                    key = f"{n}/{cls}/D{D}" + ("" if metric == "hamming" else "/" + metric)
                    if metric in skipped:
                        res["tables"][key] = {"nodes": n, "classes": cls, "distance": D, "metric": metric, "not_measured": skipped[metric]}
                        continue
                    r = {"nodes": n, "classes": cls, "distance": D, "text_bytes": len(text)}
                    if metric != "hamming":
                        r["metric"] = metric
                    r.update(dev[metric])
                    seen_ms[(cls, D, metric)] = (n, r["neighbours_device_ms"])
                    r.update(time_host_entry(classes, off, text, weights, D, a.repeats, metric))
                    if not a.no_baseline and n <= BASELINE_AT:
                        r["baseline"] = time_baseline(classes, off, text, weights, D, metric)
                        r["same_edges_and_clusters"] = (r["baseline"]["edges"] == r["stats"]["edges"] and
                                                        r["baseline"]["clusters"] == r["stats"]["clusters_out"])
                    res["tables"][key] = r
                    print(f"{key}: {r['neighbours_device_ms']} ms", file=sys.stderr, flush=True)      # (progress; the result is the JSON line)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
