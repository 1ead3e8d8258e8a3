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
Usage: tools/bench_cdr3_network.py [--sizes 100000,1000000,4000000] [--repeats 5] [--no-baseline] [--classes none,60] [--distances 1,2]"""
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


def time_device(classes, off, text, D, repeats):
    m = len(classes)
    d_cls, d_off = nat.DeviceBuffer.from_host(classes), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3net_work_bytes(m, len(text))
    d_work = nat.DeviceBuffer(wb)
    nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, None, 0, d_need, d_work, wb)
    nat.check(nat.lib().dcrx_synchronize())
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_adj = nat.DeviceBuffer(max(16, need * 4))
    e0, e1 = nat.Event(), nat.Event()
    ms = []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_neighbours_device(m, d_cls, d_off, d_text, len(text), D, d_deg, d_adj_off, d_adj, need, d_need, d_work, wb)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return {"neighbours_device_ms": round(statistics.median(ms), 3), "neighbours_device_ms_all": [round(x, 3) for x in ms],
            "adjacency_entries": need, "work_bytes": wb}


def time_host_entry(classes, off, text, weights, D, repeats):
    wall = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        _, stats = nat.cdr3_network(classes, off, text, weights, D)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"cdr3_network_ms": round(statistics.median(wall), 2), "cdr3_network_ms_all": [round(x, 2) for x in wall], "stats": stats}


def time_baseline(classes, off, text, weights, D):
    strings = cnu.node_strings(off, text)
    t0 = time.perf_counter()
    _, stats = cnu.expected_network(classes, strings, weights, D)
    return {"python_masked_search_ms": round((time.perf_counter() - t0) * 1e3, 1), "edges": stats["edges"], "clusters": stats["clusters_out"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--classes", type=str, default="none,60")
    ap.add_argument("--distances", type=str, default="1,2")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    res = {"device": nat.device_name(), "table": "11-18 residues, a fifth planted at 1-2 substitutions, seed = nodes", "repeats": a.repeats,
           "tables": {}}
    for n in (int(x) for x in a.sizes.split(",")):
        for cls in a.classes.split(","):
            classes, off, text, weights = seeded_table(n, seed=n, n_classes=1 if cls == "none" else int(cls))
            for D in (int(x) for x in a.distances.split(",")):
                r = {"nodes": n, "classes": cls, "distance": D, "text_bytes": len(text)}
                r.update(time_device(classes, off, text, D, a.repeats))
                r.update(time_host_entry(classes, off, text, weights, D, a.repeats))
                if not a.no_baseline and n <= BASELINE_AT:
                    r["baseline"] = time_baseline(classes, off, text, weights, D)
                    r["same_edges_and_clusters"] = (r["baseline"]["edges"] == r["stats"]["edges"] and
                                                    r["baseline"]["clusters"] == r["stats"]["clusters_out"])
                res["tables"][f"{n}/{cls}/D{D}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
