#!/usr/bin/env python3
"""`motifs` on the GPU: one JSON line with, for seeded tables of 10^4 and 10^5 sample units against 10^5 and 10^6 background units
(strings of 11 to 18 random residues, a planted 4-mer in 2 % of the sample), K = {2,3,4}, trim 3,3, min_count 3, at R = 100 and
R = 1000:
  - the primitive dcrx_cdr3_motifs_device on device buffers (device events), median of --repeats after a warm-up;
  - the same at R = 0: packing, the two count tables and the report alone (the steps of one call cannot be told apart by events
    from outside it: the resampling's share is the difference);
  - the host entry dcrx_cdr3_motifs as the stage calls it (wall clock, with its copies in and out), median likewise;
beside the only baseline there is, at the smallest size and --python-resamples (default 10) resamples: the contract in Python on
one thread (tests/motif_util.expected_motifs), its time per resample scaled to R.  The reported rows of both sides must agree.
--out FILE rewrites the result so far after every table.
Usage: tools/bench_cdr3_motifs.py [--samples 10000,100000] [--backgrounds 100000,1000000] [--resamples 100,1000] [--repeats 3]
                                  [--no-python] [--python-resamples 10] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402
from tests import motif_util as mu  # noqa: E402

KS, TRIM, MIN_COUNT, SEED = (2, 3, 4), (3, 3), 3, 1
WIDTH = 18


def seeded_units(count, seed, plant=0):
    """(off, text) of `count` random units; the first `plant` carry GTDT at residues 5 .. 8."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(mu.AMINO, np.uint8)
    mat, lens = letters[rng.integers(0, len(letters), (count, WIDTH))], rng.integers(11, WIDTH + 1, count)
    mat[:plant, 4:8] = np.frombuffer(b"GTDT", np.uint8)
    off = np.zeros(count + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off, mat[np.arange(WIDTH)[None, :] < lens[:, None]].tobytes()


def time_primitive(s, b, R, repeats):
    (s_off, s_text), (b_off, b_text) = s, b
    n, m = len(s_off) - 1, len(b_off) - 1
    wb = nat.cdr3_motifs_work_bytes(n, m, R)
    cap = min(n * 90, 475228)
    d_in = [nat.DeviceBuffer.from_host(x if isinstance(x, np.ndarray) else np.frombuffer(x, np.uint8)) for x in (s_off, s_text, b_off, b_text)]
    d_out = [nat.DeviceBuffer(8 * cap + 16) for _ in range(7)]
    d_need, d_stats, d_work = nat.DeviceBuffer(16), nat.DeviceBuffer(ctypes.sizeof(nat.Cdr3MotifStatsC)), nat.DeviceBuffer(wb)
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_motifs_device(n, d_in[0], d_in[1], m, d_in[2], d_in[3], KS, TRIM, MIN_COUNT, R, SEED, cap, *d_out, d_need, d_stats, d_work,
                               wb, None)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return {"device_ms": round(statistics.median(ms), 3), "device_ms_all": [round(x, 3) for x in ms],
            "reported": int(d_need.to_host(np.uint64, 1)[0]), "work_bytes": wb}


def time_host_entry(s, b, R, repeats):
    ms, out = [], None
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        out = nat.cdr3_motifs(*s, *b, KS, TRIM, MIN_COUNT, R, SEED)
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"host_entry_ms": round(statistics.median(ms), 2), "host_entry_ms_all": [round(x, 2) for x in ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", default="10000,100000")
    ap.add_argument("--backgrounds", default="100000,1000000")
    ap.add_argument("--resamples", default="100,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--python-resamples", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [(n, m) for n in map(int, a.samples.split(",")) for m in map(int, a.backgrounds.split(","))]
    result = {"bench": "cdr3_motifs", "device": nat.device_name(), "k": list(KS), "trim": list(TRIM), "min_count": MIN_COUNT, "tables": {}}
    for i, (n, m) in enumerate(sizes):
        s, b = seeded_units(n, 100 + i, plant=n // 50), seeded_units(m, 200 + i)
        row = {"counts_only": time_primitive(s, b, 0, a.repeats)}
        for R in map(int, a.resamples.split(",")):
            got, host = time_host_entry(s, b, R, a.repeats)
            row[f"R{R}"] = dict(time_primitive(s, b, R, a.repeats), **host)
            row[f"R{R}"]["resampling_ms"] = round(row[f"R{R}"]["device_ms"] - row["counts_only"]["device_ms"], 3)
            planted = [int(ge) for k, code, ge in zip(got["k"], got["code"], got["ge"]) if nat.cdr3_motif_text(int(k), int(code)) == "GTDT"]
            row[f"R{R}"]["planted_resamples_at_least"] = planted
        if i == 0 and not a.no_python:
            cut = lambda off, text: [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
            Rp = a.python_resamples
            t0 = time.perf_counter()
            want = mu.expected_motifs(cut(*s), cut(*b), KS, TRIM, MIN_COUNT, Rp, SEED)
            seconds = time.perf_counter() - t0
            t0 = time.perf_counter()
            mu.expected_motifs(cut(*s), cut(*b), KS, TRIM, MIN_COUNT, 0, SEED)
            base = time.perf_counter() - t0
            got = nat.cdr3_motifs(*s, *b, KS, TRIM, MIN_COUNT, Rp, SEED)
            mu.assert_same(got, want)
            per = (seconds - base) / max(Rp, 1)
            row["python_one_thread"] = {"resamples": Rp, "seconds": round(seconds, 2), "counts_only_seconds": round(base, 2),
                                        "seconds_per_resample": round(per, 4),
                                        **{f"scaled_to_R{R}_seconds": round(base + per * int(R), 1) for R in a.resamples.split(",")}, "agrees": True}
        result["tables"][f"{n}x{m}"] = row
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
