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
--metrics weighted times the weighted network alone (include/dcrx.h "the CDR3 network, weighted"): per table and per radius of
--radii (default 12,24) under the default cost, the primitive dcrx_cdr3_neighbours_weighted_device (device events) and the host
entry dcrx_cdr3_network_weighted (wall clock), each the median of --repeats after a warm-up with the smallest and the largest
beside it, keyed "<nodes>/<classes>/R<r>/weighted".  With --parent-tree DIR (a checkout of the parent commit with its library
built) a second process started from that tree times the parent's Levenshtein network at D = 2 on the same tables, its runs
interleaved with this process's repeat by repeat; its figures stand beside each entry under "parent_levenshtein_D2".  The same
--skip-above-s estimate applies to either side.
Usage: tools/bench_cdr3_network.py [--sizes 100000,1000000,4000000] [--repeats 5] [--no-baseline] [--classes none,60] [--distances 1,2]
                                   [--metrics hamming] [--skip-above-s 180] [--radii 12,24] [--parent-tree DIR]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 2 and sys.argv[1] == "--serve":      # the second process: this tool's loop over the PARENT's package and library
    ROOT = os.path.abspath(sys.argv[2])
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


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits),
            "all": [round(x, digits) for x in values]}


class Parent:
    """The second process: the parent commit's Levenshtein network at D = 2, one run per request."""

    def __init__(self, tree):
        import subprocess
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", tree], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True, env=dict(os.environ, DCRX_LIB_PATH=""))

    def ask(self, *words):
        self.proc.stdin.write(" ".join(str(w) for w in words) + "\n")
        self.proc.stdin.flush()
        line = self.proc.stdout.readline()
        if not line:
            raise RuntimeError("the parent's process ended")
        return json.loads(line)

    def close(self):
        self.proc.stdin.close()
        self.proc.wait()


def serve():
    """--serve: per line of standard input one step on the table named last (`table n n_classes`, `device`, `host`)."""
    state = {}
    e0, e1 = nat.Event(), nat.Event()
    for line in sys.stdin:
        w = line.split()
        if w[0] == "table":
            classes, off, text, weights = seeded_table(int(w[1]), seed=int(w[1]), n_classes=int(w[2]))
            m = len(classes)
            d = {"cls": nat.DeviceBuffer.from_host(classes), "off": nat.DeviceBuffer.from_host(off),
                 "text": nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8)), "deg": nat.DeviceBuffer(m * 4),
                 "adj_off": nat.DeviceBuffer((m + 1) * 8), "need": nat.DeviceBuffer(16)}
            wb = nat.cdr3net_work_bytes(m, len(text), metric="levenshtein")
            d["work"] = nat.DeviceBuffer(wb)
            e0.record()
            nat.cdr3_neighbours_device(m, d["cls"], d["off"], d["text"], len(text), 2, d["deg"], d["adj_off"], None, 0, d["need"], d["work"], wb,
                                       metric="levenshtein")
            e1.record()
            e1.synchronize()
            need = int(d["need"].to_host(np.uint64, 1)[0])
            d["adj"] = nat.DeviceBuffer(max(16, need * 4))
            state = {"host": (classes, off, text, weights), "dev": d, "m": m, "wb": wb, "need": need, "text_bytes": len(text)}
            out = {"adjacency_entries": need, "degree_pass_ms": e0.elapsed_ms(e1)}
        elif w[0] == "device":
            d = state["dev"]
            e0.record()
            nat.cdr3_neighbours_device(state["m"], d["cls"], d["off"], d["text"], state["text_bytes"], 2, d["deg"], d["adj_off"], d["adj"],
                                       state["need"], d["need"], d["work"], state["wb"], metric="levenshtein")
            e1.record()
            e1.synchronize()
            out = {"ms": e0.elapsed_ms(e1)}
        else:
            t0 = time.perf_counter()
            _, stats = nat.cdr3_network(*state["host"], 2, metric="levenshtein")
            out = {"ms": (time.perf_counter() - t0) * 1e3, "edges": stats["edges"]}
        print(json.dumps(out), flush=True)


def time_weighted(classes, off, text, weights, cost, R, repeats, peer):
    """The weighted primitive and host entry at one radius; after each of this process's runs the peer makes one of its own."""
    m = len(classes)
    d_cls, d_off = nat.DeviceBuffer.from_host(classes), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_adj_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3net_weighted_work_bytes(m, len(text))
    d_work = nat.DeviceBuffer(wb)
    nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, None, None, 0, d_need, d_work, wb)
    nat.check(nat.lib().dcrx_synchronize())
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_adj, d_dist = nat.DeviceBuffer(max(16, need * 4)), nat.DeviceBuffer(max(16, need * 4))
    e0, e1 = nat.Event(), nat.Event()
    ms, wall, p_ms, p_wall = [], [], [], []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, d_adj, d_dist, need, d_need, d_work, wb)
        e1.record()
        e1.synchronize()
        theirs = peer.ask("device")["ms"] if peer else None
        if k:
            ms.append(e0.elapsed_ms(e1))
            p_ms.append(theirs)
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        _, stats = nat.cdr3_network_weighted(classes, off, text, weights, cost, R)
        took = (time.perf_counter() - t0) * 1e3
        theirs = peer.ask("host") if peer else None
        if k:
            wall.append(took)
            p_wall.append(theirs)
    r = {"neighbours_device_ms": spread(ms), "adjacency_entries": need, "hits": need // 2, "work_bytes": wb,
         "cdr3_network_weighted_ms": spread(wall, 2), "stats": stats}
    if peer:
        r["parent_levenshtein_D2"] = {"neighbours_device_ms": spread(p_ms), "cdr3_network_ms": spread([x["ms"] for x in p_wall], 2),
                                      "edges": p_wall[0]["edges"]}
    return r


def main_weighted(a):
    """--metrics weighted."""
    cost = nat.Cdr3Cost.default()
    res = {"device": nat.device_name(), "table": "11-18 residues, a fifth planted at 1-2 substitutions, seed = nodes", "repeats": a.repeats,
           "cost": "default table, gap 12, trim 3,2", "figures": "median of the repeats after a warm-up, with the smallest and the largest",
           "tables": {}}
    peer = Parent(a.parent_tree) if a.parent_tree else None
    seen = {}      # (classes, radius or "parent") -> (nodes, ms) of the largest table measured so far
    walks = 2 * a.repeats + 4

    def estimate(key, n):
        before = seen.get(key)
        return (before[1] * (n / before[0]) ** 2 * walks / 1e3, before) if before else (0.0, None)
    try:
        for n in (int(x) for x in a.sizes.split(",")):
            for cls in a.classes.split(","):
                n_classes = 1 if cls == "none" else int(cls)
                classes, off, text, weights = seeded_table(n, seed=n, n_classes=n_classes)
                use_peer, why_not = peer, None
                if peer:
                    est, before = estimate((cls, "parent"), n)
                    if est > a.skip_above_s:
                        use_peer, why_not = None, f"skipped: about {est:.0f} s for its {walks} walks, from {before[1]} ms at {before[0]} nodes"
                    else:
                        peer.ask("table", n, n_classes)
                for R in (int(x) for x in a.radii.split(",")):
                    key = f"{n}/{cls}/R{R}/weighted"
                    est, before = estimate((cls, R), n)
                    if est > a.skip_above_s:
                        res["tables"][key] = {"nodes": n, "classes": cls, "radius": R, "metric": "weighted",
                                              "not_measured": f"skipped: about {est:.0f} s for its {walks} walks, from {before[1]} ms at {before[0]} nodes"}
                        continue
                    r = {"nodes": n, "classes": cls, "radius": R, "metric": "weighted", "text_bytes": len(text)}
                    r.update(time_weighted(classes, off, text, weights, cost, R, a.repeats, use_peer))
                    if why_not:
                        r["parent_levenshtein_D2"] = {"not_measured": why_not}
                    seen[(cls, R)] = (n, r["neighbours_device_ms"]["median"])
                    if use_peer:
                        seen[(cls, "parent")] = (n, r["parent_levenshtein_D2"]["neighbours_device_ms"]["median"])
                    res["tables"][key] = r
                    print(f"{key}: {r['neighbours_device_ms']['median']} ms", file=sys.stderr, flush=True)
    finally:
        if peer:
            peer.close()
    print(json.dumps(res))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--serve":
        return serve()
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--classes", type=str, default="none,60")
    ap.add_argument("--distances", type=str, default="1,2")
    ap.add_argument("--metrics", type=str, default="hamming")
    ap.add_argument("--skip-above-s", type=float, default=180.0)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--radii", type=str, default="12,24")
    ap.add_argument("--parent-tree", type=str, default=None)
    a = ap.parse_args()
    if a.metrics == "weighted":
        return main_weighted(a)
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
