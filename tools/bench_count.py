#!/usr/bin/env python3
"""The barcode-free count (`decombine -nbc --count-dcrs`) on the GPU: one JSON line with
  - the count step (dcrx_count_device, device events, median of --repeats after a warm-up) next to the decombine call
    (dcrx_decombine_device) over the same --reads reads per call, config-2 tag set, 150 nt: on dcrx_synth's reads (nearly
    all distinct) and on a skewed set (reads drawn with Zipf weights from a pool of synthetic reads; the top clone's share
    is reported);
  - the stage `decombine -nbc --count-dcrs` on --stage-reads single-end 150-nt reads from plain and from gzipped FASTQ
    (best of --stage-repeats): decombinator() by phase, and the `.nbc` write (format and file) on its own.
Usage: tools/bench_count.py [--reads 10000000] [--repeats 5] [--stage-reads 4000000] [--stage-repeats 3]"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402
from decombinator_amd import decombine as dec  # noqa: E402
from decombinator_amd import io as dio  # noqa: E402
from decombinator_amd import synth  # noqa: E402


def skewed_batch(t, n, seed, pool=20000, zipf=1.1):
    """n reads drawn with Zipf weights from `pool` synthetic reads (the decombined ones first, so the top clone counts)."""
    rng = np.random.default_rng(seed)
    b = nat.synth_reads_host(t, nat.synth_cfg(seed=seed, n_rate=0.0), 0, pool)
    rec, _ = nat.decombine(t, b)
    order = np.argsort(rec["status"] != 0, kind="stable")
    w = 1.0 / np.arange(1, pool + 1) ** zipf
    pick = order[rng.choice(pool, size=n, p=w / w.sum())]
    packed = np.ascontiguousarray(b.packed[pick])
    return nat.PackedBatch(packed, b.stride, b.read_len, None, np.zeros(0, np.uint32), np.zeros(0, np.uint16),
                           np.zeros(0, np.uint8)), float(np.bincount(pick).max()) / n


def time_step(t, batch_dev, n, repeats):
    d_rec = nat.DeviceBuffer(16 * n)
    d_cnt = nat.DeviceBuffer(8 * nat.N_COUNTERS)
    dc = nat.DcrCounts()
    e0, e1, e2 = nat.Event(), nat.Event(), nat.Event()
    dec_us, cnt_us = [], []
    distinct = 0
    for k in range(repeats + 1):
        dc.reset()
        e0.record()
        nat.decombine_device(t, batch_dev, d_rec, d_cnt)
        e1.record()
        nat.count_device(dc, d_rec, batch_dev, 0)
        e2.record()
        e2.synchronize()
        if k:                                    # (the first pass grows the table and the work space)
            dec_us.append(e0.elapsed_ms(e1) * 1e3)
            cnt_us.append(e1.elapsed_ms(e2) * 1e3)
    distinct = len(dc.read()["v"])
    hits = int(d_cnt.to_host(np.uint64, nat.N_COUNTERS)[19])
    dc.close()
    return {"decombine_us": round(statistics.median(dec_us), 1), "count_us": round(statistics.median(cnt_us), 1),
            "count_us_all": [round(x, 1) for x in cnt_us], "decombined": hits, "distinct": distinct}


def write_fastq(path, t, n, seed):
    """The reads, and beside them (`*_2.fq`) a barcode read per read for the barcoded stage over the same reads."""
    q, q2 = "I" * 150, "I" * 42
    with open(path, "w") as f, open(path.replace("_1.fq", "_2.fq"), "w") as f2:
        for a in range(0, n, 500_000):
            m = min(500_000, n - a)
            reads = nat.unpack_reads(nat.synth_reads_host(t, nat.synth_cfg(seed=seed, n_rate=0.002), a, m))
            f.write("".join(f"@SYN:{a + i} 1:N\n{r}\n+\n{q}\n" for i, r in enumerate(reads)))
            f2.write("".join(f"@SYN:{a + i} 2:N\nGTCGTGACTGGGAAAACCCTGG{(a + i) % 999983:06d}GTCGTGAT{(a + i) % 997:06d}\n+\n{q2}\n"
                             for i in range(m)))


def stage(ts, n, repeats):
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    d = tempfile.mkdtemp(prefix="nbc_bench_")
    out = {}
    try:
        ts.write(os.path.join(d, "tags"))
        write_fastq(os.path.join(d, "NBC_1.fq"), t, n, 3)
        with open(os.path.join(d, "NBC_1.fq"), "rb") as fi, gzip.open(os.path.join(d, "GZ_1.fq.gz"), "wb", compresslevel=6) as fo:
            shutil.copyfileobj(fi, fo, 16 << 20)
        cwd = os.getcwd()
        os.chdir(d)
        try:
            for name, fq in (("plain", "NBC_1.fq"), ("gz", "GZ_1.fq.gz")):
                best = None
                for _ in range(repeats):
                    # decombinator() (what §7's barcoded figure times, its `.n12` write left out) and the `.nbc` write apart
                    inp = dio.cli_args(["decombine", "-in", fq, "-br", "R2", "-nbc", "--count-dcrs", "-c", "b", "-tg", "original",
                                        "-tfdir", "tags", "-dc", "-s", "-dz", "-op", "out_"])
                    t0 = time.perf_counter()
                    data = dec.decombinator(inp)
                    t1 = time.perf_counter()
                    dio.write_out_intermediate(data, inp, dio.nbc_suffix(inp))
                    t2 = time.perf_counter()
                    if best is None or t1 - t0 < best[0]:
                        best = (t1 - t0, t2 - t1, dict(dec.stage_seconds), len(data))
                phases = {k: round(v, 3) for k, v in best[2].items()}
                phases["outside_the_loop"] = round(best[0] - sum(best[2].values()), 3)     # tag tables, FASTQ check, log
                out[name] = {"seconds": round(best[0], 3), "reads_per_s": round(n / best[0]), "phases": phases,
                             "write_nbc_seconds": round(best[1], 3), "with_write_reads_per_s": round(n / (best[0] + best[1])),
                             "distinct": best[3]}
            # the barcoded stage over the same reads (R2 barcodes beside them): decombinator() alone, its `.n12` write left out
            best = None
            for _ in range(repeats):
                inp = dio.cli_args(["decombine", "-in", "NBC_1.fq", "-br", "R2", "-c", "b", "-tg", "original", "-tfdir", "tags",
                                    "-dc", "-s", "-dz", "-op", "out_"])
                t0 = time.perf_counter()
                dec.decombinator(inp)
                dt = time.perf_counter() - t0
                if best is None or dt < best[0]:
                    best = (dt, dict(dec.stage_seconds))
            out["barcoded_plain"] = {"seconds": round(best[0], 3), "reads_per_s": round(n / best[0]),
                                     "phases": {k: round(v, 3) for k, v in best[1].items()}}
        finally:
            os.chdir(cwd)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stage-reads", type=int, default=4_000_000)
    ap.add_argument("--stage-repeats", type=int, default=3)
    a = ap.parse_args()
    ts = synth.config_tagset(2)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    res = {"device": nat.device_name(), "reads_per_call": a.reads}
    res["distinct"] = time_step(t, nat.synth_reads_device(t, nat.synth_cfg(seed=2, n_rate=0.002), 0, a.reads), a.reads, a.repeats)
    sk, top = skewed_batch(t, a.reads, 5)
    res["skewed"] = time_step(t, nat.DeviceBatch.from_host(sk), a.reads, a.repeats)
    res["skewed"]["top_clone_share"] = round(top, 4)
    del sk
    if a.stage_reads:
        res["stage"] = stage(ts, a.stage_reads, a.stage_repeats)
        res["stage"]["reads"] = a.stage_reads
        res["count_share_of_stage"] = round(res["distinct"]["count_us"] * 1e-6 * a.stage_reads / a.reads
                                            / res["stage"]["plain"]["seconds"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
