#!/usr/bin/env python3
"""The tally on the GPU (include/dcrx.h "tally, weighted"): one JSON line with, for the seeded tables of tools/bench_cdr3_match.py
(10^5 and 10^6 queries against 10^3 and 10^4 targets in 60 classes), under the default cost, each target with a radius drawn
(seeded) from the ladder 0, 2, .. 48:
  - dcrx_cdr3_tally_weighted_device: keys, sort, gather, the accumulators zeroed, one walk with a bound per target, the scatter;
  - the route it replaces, on the same tables: dcrx_cdr3_match_weighted_device at the ONE radius 48 — the degree pass that sizes
    the hit list, then the write pass into a list of exactly that size with the distances beside it — by device events, and then
    the host's part by the wall clock: the list copied back, the hits kept whose distance is within their target's own radius,
    and the totals per target; with the list's hits and bytes (8 per hit on the device), and how many of them the filter keeps;
  - a dense case, which prices the LDS adds: ONE class and one string on both sides, so every query is within every radius and
    every tested pair is a hit (10^5 queries against 10^3 targets: 10^8 adds onto the tiles' cells); the tally alone — the route
    it replaces would write a list of 10^8 hits.
Device events around the calls, median of --repeats (default 3) after a warm-up.  The two routes' totals per target are compared:
they must agree.  --out FILE rewrites the result so far after every table.  --dry checks the arguments and builds the first
table, and touches no device.
Usage: tools/bench_cdr3_tally.py [--queries 100000,1000000] [--targets 1000,10000] [--classes 60] [--radius 48] [--step 2]
                                 [--dense 100000x1000] [--repeats 3] [--dry] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decombinator_amd import _native as nat  # noqa: E402
from bench_cdr3_match import seeded_tables  # noqa: E402
from bench_cdr3_profile import timed  # noqa: E402


def ladder_radii(n_t, radius, step, seed):
    """A radius per target, drawn from 0, step, .. radius."""
    return (np.random.default_rng(seed).integers(0, radius // step + 1, n_t) * step).astype(np.uint32)


class Queries:
    def __init__(self, q):
        cls, off, text, weights = q
        self.m, self.text_bytes = len(cls), len(text)
        self.d_cls, self.d_off = nat.DeviceBuffer.from_host(cls), nat.DeviceBuffer.from_host(off)
        self.d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
        self.d_weight = nat.DeviceBuffer.from_host(np.ascontiguousarray(weights, dtype=np.uint64))

    def free(self):
        for b in (self.d_cls, self.d_off, self.d_text, self.d_weight):
            b.free()


def time_tally(index, Q, n_t, radii, cost, repeats):
    """(ms, all, t_count, t_weight, q_degree) of the primitive."""
    wb = nat.cdr3_tally_weighted_work_bytes(Q.m, Q.text_bytes, n_t)
    d_work, d_r = nat.DeviceBuffer(wb), nat.DeviceBuffer.from_host(radii)
    d_tc, d_tw, d_deg = nat.DeviceBuffer(n_t * 4), nat.DeviceBuffer(n_t * 8), nat.DeviceBuffer(Q.m * 4)
    ms, ms_all = timed(lambda: nat.cdr3_tally_weighted_device(index, Q.m, Q.d_cls, Q.d_off, Q.d_text, Q.text_bytes, Q.d_weight, cost, d_r,
                                                              d_tc, d_tw, d_deg, d_work, wb, None), repeats)
    out = d_tc.to_host(np.uint32, n_t), d_tw.to_host(np.uint64, n_t), d_deg.to_host(np.uint32, Q.m)
    for b in (d_work, d_r, d_tc, d_tw, d_deg):
        b.free()
    return (ms, ms_all, wb) + out


def time_match_route(index, Q, n_t, radii, weights, cost, radius, repeats):
    """The route the tally replaces: (device ms, all, host ms, hits, kept, t_count, t_weight)."""
    m = Q.m
    wb = nat.cdr3_match_weighted_work_bytes(m, Q.text_bytes)
    d_work, d_deg, d_hit_off, d_need = nat.DeviceBuffer(wb), nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
    nat.cdr3_match_weighted_device(index, m, Q.d_cls, Q.d_off, Q.d_text, Q.text_bytes, cost, radius, d_deg, d_hit_off, None, None, 0, d_need,
                                   d_work, wb, None)
    nat.synchronize()
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_hit, d_dist = nat.DeviceBuffer(max(need, 1) * 4), nat.DeviceBuffer(max(need, 1) * 4)

    def both_passes():      # (the sizing call, then the call that writes: what a caller without the need makes)
        nat.cdr3_match_weighted_device(index, m, Q.d_cls, Q.d_off, Q.d_text, Q.text_bytes, cost, radius, d_deg, d_hit_off, None, None, 0, d_need,
                                       d_work, wb, None)
        nat.cdr3_match_weighted_device(index, m, Q.d_cls, Q.d_off, Q.d_text, Q.text_bytes, cost, radius, d_deg, d_hit_off, d_hit, d_dist, need,
                                       d_need, d_work, wb, None)
    ms, ms_all = timed(both_passes, repeats)
    t0 = time.perf_counter()
    hit, dist = d_hit.to_host(np.uint32, max(need, 1))[:need].astype(np.int64), d_dist.to_host(np.uint32, max(need, 1))[:need]
    hit_off = d_hit_off.to_host(np.uint64, m + 1).astype(np.int64)
    owner = np.repeat(np.arange(m, dtype=np.int64), np.diff(hit_off))
    keep = dist <= radii[hit]
    t_count = np.bincount(hit[keep], minlength=n_t).astype(np.uint32)
    t_weight = np.zeros(n_t, np.uint64)
    np.add.at(t_weight, hit[keep], weights[owner[keep]])
    host_ms = round((time.perf_counter() - t0) * 1e3, 3)
    for b in (d_work, d_deg, d_hit_off, d_need, d_hit, d_dist):
        b.free()
    return ms, ms_all, host_ms, need, int(keep.sum()), t_count, t_weight


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=str, default="100000,1000000")
    ap.add_argument("--targets", type=str, default="1000,10000")
    ap.add_argument("--classes", type=int, default=60)
    ap.add_argument("--radius", type=int, default=48)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--dense", type=str, default="100000x1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not 0 <= a.radius <= 65535 or a.step < 1 or a.radius % a.step or a.repeats < 1 or a.classes < 1:
        raise SystemExit("--radius is 0 .. 65535 and a multiple of --step, --repeats and --classes 1 or more")
    shapes = list(itertools.product((int(x) for x in a.queries.split(",")), (int(x) for x in a.targets.split(","))))
    dense = tuple(int(x) for x in a.dense.split("x")) if a.dense else None
    if a.dry:
        n_q, n_t = shapes[0]
        t, q = seeded_tables(min(n_q, 1000), min(n_t, 1000), a.classes, seed=n_q + n_t)
        print(json.dumps({"dry": True, "shapes": [f"{x}x{y}/{a.classes}" for x, y in shapes], "dense": dense, "radius": a.radius, "step": a.step,
                          "first_table": [len(q[0]), len(t[0])], "first_radii": ladder_radii(len(t[0]), a.radius, a.step, 1)[:8].tolist()}))
        return
    cost = nat.Cdr3Cost.default()
    res = {"device": nat.device_name(), "radius": a.radius, "step": a.step, "repeats": a.repeats, "gap": cost.gap, "trim": [cost.ntrim, cost.ctrim],
           "table": "tools/bench_cdr3_match.py seeded_tables: 11-18 residues; a fifth of the queries planted 0-2 edits from a target; "
                    "seed = queries + targets; a radius per target drawn from 0, step, .. radius with the same seed", "tables": {}}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    for n_q, n_t in shapes:
        t, q = seeded_tables(n_q, n_t, a.classes, seed=n_q + n_t)
        radii = ladder_radii(n_t, a.radius, a.step, n_q + n_t)
        index, Q = nat.Cdr3Index(*t), Queries(q)
        r = {"queries": n_q, "targets": n_t, "classes": a.classes}
        r["tally_ms"], r["tally_ms_all"], r["tally_work_bytes"], tc, tw, deg = time_tally(index, Q, n_t, radii, cost, a.repeats)
        r["tally_hits"], r["tally_queries_inside"] = int(tc.astype(np.uint64).sum()), int((deg > 0).sum())
        (r["match_two_passes_ms"], r["match_two_passes_ms_all"], r["match_host_filter_ms"], r["match_hits_listed"], r["match_hits_kept"],
         mc, mw) = time_match_route(index, Q, n_t, radii, np.ascontiguousarray(q[3], dtype=np.uint64), cost, a.radius, a.repeats)
        r["match_hit_list_bytes"] = 8 * r["match_hits_listed"]
        r["same_totals"] = bool(np.array_equal(tc, mc) and np.array_equal(tw, mw) and r["tally_hits"] == r["match_hits_kept"])
        r["tally_over_match_device"] = round(r["tally_ms"] / r["match_two_passes_ms"], 3)
        res["tables"][f"{n_q}x{n_t}/{a.classes}"] = r
        print(f"{n_q}x{n_t}/{a.classes}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
        index.close()
        Q.free()
    if dense:
        n_q, n_t = dense
        s = b"CASSLAPGATNEKLF"
        spans = lambda n: (np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64) * len(s), s * n)
        index, Q = nat.Cdr3Index(*spans(n_t)), Queries(spans(n_q) + (np.full(n_q, 3, np.uint64),))
        radii = ladder_radii(n_t, a.radius, a.step, n_q + n_t)
        r = {"queries": n_q, "targets": n_t, "classes": 1, "pairs": n_q * n_t}
        r["tally_ms"], r["tally_ms_all"], r["tally_work_bytes"], tc, tw, deg = time_tally(index, Q, n_t, radii, cost, a.repeats)
        r["every_pair_counted"] = bool((tc == n_q).all() and (tw == 3 * n_q).all() and (deg == n_t).all())
        r["ns_per_pair"] = round(r["tally_ms"] * 1e6 / r["pairs"], 4)
        res["dense"] = r
        print("dense: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        save()
        index.close()
        Q.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
