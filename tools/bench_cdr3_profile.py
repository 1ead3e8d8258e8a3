#!/usr/bin/env python3
"""The radius profile on the GPU (include/dcrx.h "profile, weighted"): one JSON line with, for the seeded tables of
tools/bench_cdr3_match.py (10^5 and 10^6 queries against 10^5 and 10^6 targets in 60 classes; under class `none` 10^5 against 10^5
only), under the default cost:
  - the figure the new sink is set against: the weighted match's own walk at the ladder's top, the degree pass of
    dcrx_cdr3_match_weighted_device at radius R = 48 with hit_cap 0 (keys, sort, gather, one walk that counts, the scan);
  - dcrx_cdr3_profile_weighted_device at (step 2, bins 25) and at (step 48, bins 2): keys, sort, gather, one walk that bins;
  - each profile's ratio to that degree pass, and 25 times the degree pass: what the ladder costs through the entries there were.
Device events around the call, median of --repeats (default 3) after a warm-up.  The sum of every profile's cells is compared
with the degree pass's need (the pairs within R): they must agree.  --out FILE rewrites the result so far after every table.
--dry checks the arguments and builds the first table, and touches no device.
Usage: tools/bench_cdr3_profile.py [--queries 100000,1000000] [--targets 100000,1000000] [--classes 60,none] [--radius 48]
                                   [--ladders 2x25,48x2] [--repeats 3] [--dry] [--out FILE]"""
import argparse
import itertools
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decombinator_amd import _native as nat  # noqa: E402
from bench_cdr3_match import seeded_tables  # noqa: E402

NONE_AT = (100_000, 100_000)      # the only table that runs under class `none`


def timed(call, repeats):
    """(median, all) of the call's device time in ms, after a warm-up."""
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def parse_ladders(text, radius):
    out = []
    for word in text.split(","):
        step, bins = (int(x) for x in word.split("x"))
        if not (1 <= step <= 65535 and 1 <= bins <= nat.CDR3_PROFILE_MAX_BINS and step * (bins - 1) == radius):
            raise SystemExit(f"--ladders: {word} is not STEPxBINS with 1 <= BINS <= 32 and STEP * (BINS - 1) = --radius ({radius})")
        out.append((step, bins))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=str, default="100000,1000000")
    ap.add_argument("--targets", type=str, default="100000,1000000")
    ap.add_argument("--classes", type=str, default="60,none")
    ap.add_argument("--radius", type=int, default=48)
    ap.add_argument("--ladders", type=str, default="2x25,48x2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not 0 <= a.radius <= 65535 or a.repeats < 1:
        raise SystemExit("--radius is 0 .. 65535 and --repeats 1 or more")
    ladders = parse_ladders(a.ladders, a.radius)
    shapes = [(n_q, n_t, cls) for n_q, n_t, cls in itertools.product((int(x) for x in a.queries.split(",")),
                                                                    (int(x) for x in a.targets.split(",")), a.classes.split(","))
              if cls != "none" or (n_q, n_t) == NONE_AT]
    if a.dry:
        n_q, n_t, cls = shapes[0]
        t, q = seeded_tables(min(n_q, 1000), min(n_t, 1000), 1 if cls == "none" else int(cls), seed=n_q + n_t)
        print(json.dumps({"dry": True, "shapes": [f"{x}x{y}/{c}" for x, y, c in shapes], "ladders": ladders, "radius": a.radius,
                          "first_table": [len(q[0]), len(t[0])]}))
        return
    cost = nat.Cdr3Cost.default()
    res = {"device": nat.device_name(), "radius": a.radius, "repeats": a.repeats, "gap": cost.gap, "trim": [cost.ntrim, cost.ctrim],
           "table": "tools/bench_cdr3_match.py seeded_tables: 11-18 residues; a fifth of the queries planted 0-2 edits from a target; "
                    "seed = queries + targets", "tables": {}}
    for n_q, n_t, cls in shapes:
        t, (q_cls, q_off, q_text, _) = seeded_tables(n_q, n_t, 1 if cls == "none" else int(cls), seed=n_q + n_t)
        index = nat.Cdr3Index(*t)
        m = len(q_cls)
        d_cls, d_off = nat.DeviceBuffer.from_host(q_cls), nat.DeviceBuffer.from_host(q_off)
        d_text = nat.DeviceBuffer.from_host(np.frombuffer(q_text + b"\0", np.uint8))
        d_deg, d_hit_off, d_need = nat.DeviceBuffer(m * 4), nat.DeviceBuffer((m + 1) * 8), nat.DeviceBuffer(16)
        wb = nat.cdr3_match_weighted_work_bytes(m, len(q_text))
        d_work = nat.DeviceBuffer(wb)
        r = {"queries": n_q, "targets": n_t, "classes": cls}
        r["degree_pass_ms"], r["degree_pass_ms_all"] = timed(lambda: nat.cdr3_match_weighted_device(
            index, m, d_cls, d_off, d_text, len(q_text), cost, a.radius, d_deg, d_hit_off, None, None, 0, d_need, d_work, wb, None), a.repeats)
        r["pairs_within_radius"] = int(d_need.to_host(np.uint64, 1)[0])
        r["ladder_by_degree_passes_ms"] = round(25 * r["degree_pass_ms"], 3)
        r["same_sums"] = True
        for step, bins in ladders:
            pb = nat.cdr3_profile_weighted_work_bytes(m, len(q_text), bins)
            d_pwork, d_profile = nat.DeviceBuffer(pb), nat.DeviceBuffer(m * bins * 4)
            ms, ms_all = timed(lambda: nat.cdr3_profile_weighted_device(index, m, d_cls, d_off, d_text, len(q_text), cost, step, bins,
                                                                        d_profile, d_pwork, pb, None), a.repeats)
            total = int(d_profile.to_host(np.uint32, m * bins).astype(np.uint64).sum())
            r[f"profile_{step}x{bins}_ms"], r[f"profile_{step}x{bins}_ms_all"] = ms, ms_all
            r[f"profile_{step}x{bins}_over_degree_pass"] = round(ms / r["degree_pass_ms"], 3)
            r["same_sums"] = r["same_sums"] and total == r["pairs_within_radius"]
            d_pwork.free(); d_profile.free()
        res["tables"][f"{n_q}x{n_t}/{cls}"] = r
        print(f"{n_q}x{n_t}/{cls}: " + ", ".join(f"{k} {v}" for k, v in r.items() if not k.endswith("_all")), file=sys.stderr, flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
        index.close()
        for b in (d_cls, d_off, d_text, d_deg, d_hit_off, d_need, d_work):
            b.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
