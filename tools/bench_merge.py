#!/usr/bin/env python3
"""The error merge of the barcode-free count (`--merge-errors`) on the GPU: one JSON line with, for (a) noisy clonal reads
(Zipf-weighted copies of a pool of pristine synthetic reads, every copy with its own substitutions) and (b) dcrx_synth's
nearly distinct reads, config-2 tag set, 150 nt:
  - the merge step alone on the table counted from --reads reads: dcrx_merge_dcrs (wall clock, with its copies in and out)
    and the primitive dcrx_merge_parents_device on device buffers (device events), median of --repeats after a warm-up;
    with --brute the contract's Python brute force (tests/nbc_merge_util.expected_merge) on the same table;
  - the stage `decombine -nbc --count-dcrs` over --stage-reads reads of plain FASTQ with and without --merge-errors, best of
    --stage-repeats, interleaved.
Usage: tools/bench_merge.py [--reads 10000000] [--repeats 5] [--stage-reads 4000000] [--stage-repeats 3] [--brute]"""
import argparse
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

CHUNK = 1_000_000


def noisy_batch(t, first, n, seed, pool=20000, zipf=1.1, sub_rate=0.005):
    """n packed reads: Zipf-weighted copies of `pool` pristine synthetic reads (the decombined ones first), every copy with
    its own substitutions at sub_rate per base (a 2-bit field XORed with 1 .. 3: another base, never the same)."""
    rng = np.random.default_rng((seed, first))
    b = nat.synth_reads_host(t, nat.synth_cfg(seed=seed, p_rearranged=0.9, sub_rate=0.0, n_rate=0.0), 0, pool)
    rec, _ = nat.decombine(t, b)
    order = np.argsort(rec["status"] != 0, kind="stable")
    w = 1.0 / np.arange(1, pool + 1) ** zipf
    packed = np.ascontiguousarray(b.packed[order[rng.choice(pool, size=n, p=w / w.sum())]])
    hits = int(rng.binomial(n * b.read_len, sub_rate))
    rows, cols = rng.integers(0, n, hits), rng.integers(0, b.read_len, hits)
    delta = (rng.integers(1, 4, hits) << (2 * (cols % 4))).astype(np.uint8)
    np.bitwise_xor.at(packed.reshape(-1), rows * b.stride + cols // 4, delta)
    return nat.PackedBatch(packed, b.stride, b.read_len, None, np.zeros(0, np.uint32), np.zeros(0, np.uint16), np.zeros(0, np.uint8))


def batches(t, kind, n):
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        yield a, (noisy_batch(t, a, m, 7) if kind == "noisy" else nat.synth_reads_host(t, nat.synth_cfg(seed=2, n_rate=0.002), a, m))


def counted_table(t, kind, n):
    dc = nat.DcrCounts()
    for a, b in batches(t, kind, n):
        nat.decombine_count(t, b, dc, a)
    counted = dc.read()
    dc.close()
    return counted


def time_merge(t, counted, repeats, D, R):
    n = len(counted["v"])
    wall = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        out, stats, _ = nat.merge_dcrs(t, counted, D, R)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    bufs = [nat.DeviceBuffer.from_host(counted[f]) for f in ("v", "j", "vdel", "jdel", "count", "ins_off")]
    text = np.frombuffer(counted["ins_text"], np.uint8)
    d_text = nat.DeviceBuffer.from_host(text)
    wb = int(nat.lib().dcrx_merge_work_bytes(n))
    d_work, d_parent, d_reach = nat.DeviceBuffer(wb), nat.DeviceBuffer(4 * n), nat.DeviceBuffer(n)
    e0, e1 = nat.Event(), nat.Event()
    dev = []
    for k in range(repeats + 1):
        e0.record()
        nat.merge_parents_device(t, n, *bufs, d_text, len(text), D, R, d_parent, d_reach, d_work, wb)
        e1.record()
        e1.synchronize()
        if k:
            dev.append(e0.elapsed_ms(e1))
    return {"entries": n, "count_1_entries": int((counted["count"] == 1).sum()), "stats": stats,
            "merge_dcrs_ms": round(statistics.median(wall), 2), "merge_dcrs_ms_all": [round(x, 2) for x in wall],
            "parents_device_ms": round(statistics.median(dev), 3), "parents_device_ms_all": [round(x, 3) for x in dev],
            "table_gather_ms_note": "merge_dcrs_ms includes the copies in and out and the host gather of the roots' keys"}


def stage(ts, t, kind, n, repeats):
    d = tempfile.mkdtemp(prefix="merge_bench_")
    try:
        ts.write(os.path.join(d, "tags"))
        q = "I" * 150
        with open(os.path.join(d, "NBC_1.fq"), "w") as f:
            for a, b in batches(t, kind, n):
                f.write("".join(f"@SYN:{a + i} 1:N\n{r}\n+\n{q}\n" for i, r in enumerate(nat.unpack_reads(b))))
        cwd = os.getcwd()
        os.chdir(d)
        try:
            best = {}
            for _ in range(repeats):
                for name, extra in (("count_only", []), ("merge_errors", ["--merge-errors"])):
                    inp = dio.cli_args(["decombine", "-in", "NBC_1.fq", "-br", "R2", "-nbc", "--count-dcrs", "-c", "b", "-tg", "original",
                                        "-tfdir", "tags", "-dc", "-s", "-dz", "-op", "out_"] + extra)
                    t0 = time.perf_counter()
                    data = dec.decombinator(inp)
                    dt = time.perf_counter() - t0
                    if name not in best or dt < best[name][0]:
                        best[name] = (dt, dict(dec.stage_seconds), len(data))
            return {name: {"seconds": round(v[0], 3), "reads_per_s": round(n / v[0]), "phases": {k: round(x, 3) for k, x in v[1].items()},
                           "rows": v[2]} for name, v in best.items()}
        finally:
            os.chdir(cwd)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stage-reads", type=int, default=4_000_000)
    ap.add_argument("--stage-repeats", type=int, default=3)
    ap.add_argument("--distance", type=int, default=1)
    ap.add_argument("--ratio", type=int, default=10)
    ap.add_argument("--brute", action="store_true", help="also time the Python brute force on the same tables (slow)")
    a = ap.parse_args()
    ts = synth.config_tagset(2)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    res = {"device": nat.device_name(), "reads": a.reads, "distance": a.distance, "ratio": a.ratio}
    for kind in ("noisy", "distinct"):
        counted = counted_table(t, kind, a.reads)
        r = time_merge(t, counted, a.repeats, a.distance, a.ratio)
        if a.brute:
            from tests import nbc_merge_util as nm
            t0 = time.perf_counter()
            nm.expected_merge(counted, ts, a.distance, a.ratio)
            r["python_brute_force_s"] = round(time.perf_counter() - t0, 2)
        del counted
        if a.stage_reads:
            r["stage"] = stage(ts, t, kind, a.stage_reads, a.stage_repeats)
            r["stage"]["reads"] = a.stage_reads
            r["merge_share_of_stage"] = round(r["stage"]["merge_errors"]["phases"].get("merge", 0.0) / r["stage"]["merge_errors"]["seconds"], 4)
        res[kind] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
