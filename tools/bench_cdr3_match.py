#!/usr/bin/env python3
"""`match` on the GPU: one JSON line with, for seeded tables of 10^5 and 10^6 queries against 10^4 and 10^5 targets (strings of
11 to 18 random residues; a fifth of the queries planted 0 to 2 edits — substitutions, and one in three an insertion or a
deletion — from a target and in its class; Zipf-like weights), under class `none` and under 60 classes, for both metrics at
--distance (default 1):
  - the index build dcrx_cdr3_index_create (wall clock, with its upload), median of --repeats after a warm-up;
  - the primitive dcrx_cdr3_match_device on device buffers with hits of the exact size (device events), median likewise;
  - the host entry dcrx_cdr3_match_run as the stage calls it (wall clock, with its copies in and out), median likewise;
beside two baselines that give the same hits:
  - the route there was before: dcrx_cdr3_network_metric with edges over the two tables concatenated, and the cross edges
    filtered out on the host (wall clock; where its warm-up alone takes more than --slow-s seconds that one run is the figure
    and "runs" says 1; where the quadratic estimate from a smaller table of the same classes and metric is above
    --skip-above-s it is not run and says so);
  - at 10^5 queries against 10^4 targets only, a Python search on one thread: the targets entered under their strings with D
    positions masked (Hamming) or up to D bytes deleted (Levenshtein, candidates verified by the edit-distance table).
Every side's hit count is compared: they must agree.  --out FILE rewrites the result so far after every table.
--metrics may also name `weighted` (include/dcrx.h "match, weighted"): the same seeded tables under the default cost at R = 12
and at R = 24 (keys .../weighted12 and .../weighted24), the primitive and the host entry timed likewise; the network route does
not exist for it, and its only baseline is --python-util: tests/cdr3_wmatch_util.expected_numpy (the literal minimum over every
gap position, as array operations, on one thread) at 10^5 queries against 10^4 targets where the classes are not `none` (all
pairs of 10^9 are not run).  --python-util needs no GPU when given with --no-gpu.
Usage: tools/bench_cdr3_match.py [--queries 100000,1000000] [--targets 10000,100000] [--classes none,60]
                                 [--metrics hamming,levenshtein,weighted] [--distance 1] [--repeats 5] [--no-baselines] [--slow-s 20]
                                 [--skip-above-s 120] [--python-util] [--no-gpu] [--out FILE]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402
from tests import cdr3_match_util as mu  # noqa: E402
from tests import cdr3_network_util as cnu  # noqa: E402
from tests import cdr3_wmatch_util as wu  # noqa: E402

PYTHON_AT = (100_000, 10_000)
WEIGHTED_RADII = (12, 24)
WIDTH = 18


def _spans(mat, lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off, mat[np.arange(mat.shape[1])[None, :] < lens[:, None]].tobytes()


def seeded_tables(n_q, n_t, n_classes, seed):
    """((target classes, off, text), (query classes, off, text, weights))."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(cnu.AMINO.encode(), np.uint8)
    draw = lambda n: (letters[rng.integers(0, len(letters), (n, WIDTH + 1))], rng.integers(11, WIDTH + 1, n),
                      rng.integers(0, n_classes, n).astype(np.uint32) if n_classes > 1 else np.zeros(n, np.uint32))
    (t_mat, t_len, t_cls), (q_mat, q_len, q_cls) = draw(n_t), draw(n_q)
    planted = rng.choice(n_q, n_q // 5, replace=False)
    src = rng.integers(0, n_t, len(planted))
    q_mat[planted], q_len[planted], q_cls[planted] = t_mat[src], t_len[src], t_cls[src]
    for k in range(2):      # a substitution for two in three of them, a second for one in three
        hit = planted[rng.random(len(planted)) < (2 / 3 if k == 0 else 1 / 3)]
        q_mat[hit, rng.integers(0, q_len[hit])] = letters[rng.integers(0, len(letters), len(hit))]
    for i in planted[rng.random(len(planted)) < 1 / 3].tolist():      # an insertion or a deletion
        n, p = int(q_len[i]), int(rng.integers(0, q_len[i]))
        row = q_mat[i, :n].tolist()
        if rng.random() < 0.5 and n > 11:
            del row[p]
        elif n < WIDTH:
            row.insert(p, int(letters[rng.integers(0, len(letters))]))
        q_mat[i, :len(row)], q_len[i] = row, len(row)
    weights = np.sort(np.maximum(1, (1000 / (1 + rng.pareto(1.2, n_q) * 20)).astype(np.uint64)))[::-1].copy()
    return (t_cls, *_spans(t_mat, t_len)), (q_cls, *_spans(q_mat, q_len), weights)


def median_after_warm_up(call, repeats):
    ms = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        out = call()
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, round(statistics.median(ms), 2), [round(x, 2) for x in ms]


def time_primitive(index, q, D, metric, repeats):
    cls, off, text, _ = q
    m = len(cls)
    d_cls, d_off = nat.DeviceBuffer.from_host(cls), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_hit_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3_match_work_bytes(m, len(text), metric)
    d_work = nat.DeviceBuffer(wb)
    nat.cdr3_match_device(index, m, d_cls, d_off, d_text, len(text), D, d_deg, d_hit_off, None, 0, d_need, d_work, wb, None, metric)
    nat.check(nat.lib().dcrx_synchronize())
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_hit = nat.DeviceBuffer(max(16, need * 4))
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_match_device(index, m, d_cls, d_off, d_text, len(text), D, d_deg, d_hit_off, d_hit, need, d_need, d_work, wb, None, metric)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return {"match_device_ms": round(statistics.median(ms), 3), "match_device_ms_all": [round(x, 3) for x in ms], "hits": need,
            "work_bytes": wb}


def time_weighted_primitive(index, q, cost, R, repeats):
    """time_primitive for dcrx_cdr3_match_weighted_device, the hits' distances written too."""
    cls, off, text, _ = q
    m = len(cls)
    d_cls, d_off = nat.DeviceBuffer.from_host(cls), nat.DeviceBuffer.from_host(off)
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_deg, d_hit_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    wb = nat.cdr3_match_weighted_work_bytes(m, len(text))
    d_work = nat.DeviceBuffer(wb)
    args = (index, m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_hit_off)
    nat.cdr3_match_weighted_device(*args, None, None, 0, d_need, d_work, wb, None)
    nat.check(nat.lib().dcrx_synchronize())
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_hit, d_dist = nat.DeviceBuffer(max(16, need * 4)), nat.DeviceBuffer(max(16, need * 4))
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_match_weighted_device(*args, d_hit, d_dist, need, d_need, d_work, wb, None)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return {"match_device_ms": round(statistics.median(ms), 3), "match_device_ms_all": [round(x, 3) for x in ms], "hits": need,
            "work_bytes": wb}


def python_util(t, q, cost, R):
    """(hits, seconds) of the Python contract in its numpy form, on one thread."""
    (t_cls, t_off, t_text), (q_cls, q_off, q_text, w) = t, q
    case = mu.Case(t_cls.tolist(), cnu.node_strings(t_off, t_text), q_cls.tolist(), cnu.node_strings(q_off, q_text), w.tolist())
    t0 = time.perf_counter()
    hits = wu.expected_numpy(case, cost, R)["stats"]["hits"]
    return hits, time.perf_counter() - t0


def network_route(t, q, D, metric):
    """The hits by the route there was before: the network over queries + targets, the cross edges kept."""
    (t_cls, t_off, t_text), (q_cls, q_off, q_text, w) = t, q
    n_q = len(q_cls)
    classes = np.concatenate([q_cls, t_cls])
    off = np.concatenate([q_off, t_off[1:] + q_off[-1]])
    net, _ = nat.cdr3_network(classes, off, q_text + t_text, np.concatenate([w, np.ones(len(t_cls), np.uint64)]), D, want_edges=True,
                              metric=metric)
    rows = np.repeat(np.arange(len(classes)), np.diff(net["adj_off"]).astype(np.int64))
    return int(np.count_nonzero((rows < n_q) & (net["adj"] >= n_q)))


def python_search(t, q, D, metric):
    """The hits by a dictionary search on one thread."""
    (t_cls, t_off, t_text), (q_cls, q_off, q_text, _) = t, q
    ts, qs = cnu.node_strings(t_off, t_text), cnu.node_strings(q_off, q_text)
    if metric == "hamming":
        masks = lambda s: [s] if D == 0 else [s[:p] + b"\0" + s[p + 1:] for p in range(len(s))] if D == 1 else \
            [s[:a] + b"\0" + s[a + 1:b] + b"\0" + s[b + 1:] for a, b in itertools.combinations(range(len(s)), 2)]
        near = lambda a, b: True
    else:
        masks = lambda s: mu._deletions(s, D)
        near = lambda a, b: mu.lev(a, b) <= D
    table = {}
    for j, s in enumerate(ts):
        for v in masks(s):
            table.setdefault((int(t_cls[j]), v), []).append(j)
    hits = 0
    for i, s in enumerate(qs):
        c = int(q_cls[i])
        found = set()
        for v in masks(s):
            found.update(table.get((c, v), ()))
        hits += sum(1 for j in found if near(s, ts[j]))
    return hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=str, default="100000,1000000")
    ap.add_argument("--targets", type=str, default="10000,100000")
    ap.add_argument("--classes", type=str, default="none,60")
    ap.add_argument("--metrics", type=str, default="hamming,levenshtein")
    ap.add_argument("--distance", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--slow-s", type=float, default=20.0)
    ap.add_argument("--skip-above-s", type=float, default=120.0)
    ap.add_argument("--python-util", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    D = a.distance
    res = {"device": None if a.no_gpu else nat.device_name(), "distance": D, "repeats": a.repeats,
           "table": "11-18 residues; a fifth of the queries planted 0-2 edits from a target; seed = queries + targets", "tables": {}}
    seen = {}      # (classes, metric) -> (nodes, seconds) of the slowest network route run so far
    for n_q, n_t, cls in itertools.product((int(x) for x in a.queries.split(",")), (int(x) for x in a.targets.split(",")), a.classes.split(",")):
        t, q = seeded_tables(n_q, n_t, 1 if cls == "none" else int(cls), seed=n_q + n_t)
        if a.no_gpu:
            for R in WEIGHTED_RADII if a.python_util and (n_q, n_t) == PYTHON_AT and cls != "none" else ():
                hits, s = python_util(t, q, nat.Cdr3Cost.default(), R)
                res["tables"][f"{n_q}x{n_t}/{cls}/weighted{R}"] = {"python_util_hits": hits, "python_util_s": round(s, 1)}
            continue
        index, build_ms, build_all = median_after_warm_up(lambda: nat.Cdr3Index(*t), a.repeats)
        for metric, R in [(m, R) for m in a.metrics.split(",") for R in (WEIGHTED_RADII if m == "weighted" else (None,))]:
            if metric == "weighted":
                cost = nat.Cdr3Cost.default()
                key = f"{n_q}x{n_t}/{cls}/weighted{R}"
                r = {"queries": n_q, "targets": n_t, "classes": cls, "metric": metric, "radius": R, "gap": cost.gap, "trim": [cost.ntrim, cost.ctrim],
                     "index_create_ms": build_ms, "index_create_ms_all": build_all, "index_bytes": index.info()["device_bytes"]}
                r.update(time_weighted_primitive(index, q, cost, R, a.repeats))
                out, r["match_run_ms"], r["match_run_ms_all"] = median_after_warm_up(lambda: nat.cdr3_match_weighted(index, *q, cost, R), a.repeats)
                r["stats"] = out["stats"]
                r["same_hits"] = out["stats"]["hits"] == r["hits"]
                if a.python_util and (n_q, n_t) == PYTHON_AT and cls != "none":
                    hits, s = python_util(t, q, cost, R)
                    r["python_util_s"], r["same_hits"] = round(s, 1), r["same_hits"] and hits == r["hits"]
                res["tables"][key] = r
                print(f"{key}: device {r['match_device_ms']} ms, run {r['match_run_ms']} ms, {r['hits']} hits", file=sys.stderr, flush=True)
                if a.out:
                    with open(a.out, "w") as fh:
                        fh.write(json.dumps(res) + "\n")
                continue
            key = f"{n_q}x{n_t}/{cls}/{metric}"
            r = {"queries": n_q, "targets": n_t, "classes": cls, "metric": metric, "index_create_ms": build_ms, "index_create_ms_all": build_all,
                 "index_bytes": index.info()["device_bytes"]}
            r.update(time_primitive(index, q, D, metric, a.repeats))
            out, r["match_run_ms"], r["match_run_ms_all"] = median_after_warm_up(lambda: nat.cdr3_match(index, *q, D, metric), a.repeats)
            r["stats"] = out["stats"]
            same = out["stats"]["hits"] == r["hits"]
            if not a.no_baselines:
                before = seen.get((cls, metric))
                estimate = before[1] * ((n_q + n_t) / before[0]) ** 2 if before else 0.0
                if estimate > a.skip_above_s:
                    r["network_route"] = f"not run: about {estimate:.0f} s a run, from {before[1]:.1f} s at {before[0]} nodes"
                else:
                    t0 = time.perf_counter()
                    hits = network_route(t, q, D, metric)
                    first = time.perf_counter() - t0
                    if first > a.slow_s:
                        r["network_route_ms"], r["network_route_runs"] = round(first * 1e3, 1), 1
                    else:
                        _, r["network_route_ms"], r["network_route_ms_all"] = median_after_warm_up(lambda: network_route(t, q, D, metric),
                                                                                                 a.repeats)
                        r["network_route_runs"] = a.repeats
                    seen[(cls, metric)] = (n_q + n_t, r["network_route_ms"] / 1e3)
                    same = same and hits == r["hits"]
                if (n_q, n_t) == PYTHON_AT:
                    t0 = time.perf_counter()
                    hits = python_search(t, q, D, metric)
                    r["python_search_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    same = same and hits == r["hits"]
            r["same_hits"] = same
            res["tables"][key] = r
            print(f"{key}: device {r['match_device_ms']} ms, run {r['match_run_ms']} ms, route {r.get('network_route_ms', r.get('network_route'))}",
                  file=sys.stderr, flush=True)      # (progress; the result is the JSON line)
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(res) + "\n")
        index.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
