#!/usr/bin/env python3
"""Stage 2 of `collapse` on the GPU: one JSON line with the UMI neighbour search kernel's time (device events around
dcrx_umi_neighbours_device after a warm-up launch) and pair count for seeded synthetic 12-nt UMIs with planted families at
k = 2, the whole `collapse --cluster` over synthetic rows split by stage, and beside the kernel a CPU baseline (an
independent neighbour search, tests/collapse_cluster_util.symdel_neighbours, labelled as such; one thread, on the smallest
size only).  Usage: tools/bench_collapse.py [--sizes 100000,1000000,4000000] [--rows 1000000] [--cpu-baseline]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402


def synth_umis(n, seed):
    """n distinct 12-nt UMIs: random bases, a quarter of them one substitution away from another (planted families)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, 12), dtype=np.uint8)
    fam = rng.random(n) < 0.25
    src = rng.integers(0, n, size=n)
    codes[fam] = codes[src[fam]]
    pos = rng.integers(0, 12, size=n)
    codes[fam, pos[fam]] = (codes[fam, pos[fam]] + rng.integers(1, 4, size=int(fam.sum()), dtype=np.uint8)) % 4
    raw = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    uniq = np.unique(raw.view("S12").ravel())
    rng.shuffle(uniq)
    text = uniq.tobytes()
    off = np.arange(len(uniq) + 1, dtype=np.uint64) * 12
    return text, off


def kernel_ms(text, off, k, reps=3):
    n = len(off) - 1
    t = np.frombuffer(text, dtype=np.uint8)
    n_tiles = nat.check(nat.lib().dcrx_umi_encode(t.ctypes.data, off.ctypes.data, n, None, None))
    recs = np.zeros(n_tiles * nat.UMI_TILE * nat.UMI_REC_WORDS, dtype=np.uint32)
    tiles = np.zeros(n_tiles * nat.UMI_TILE_WORDS, dtype=np.uint32)
    t0 = time.time()
    nat.check(nat.lib().dcrx_umi_encode(t.ctypes.data, off.ctypes.data, n, recs.ctypes.data, tiles.ctypes.data))
    encode_s = time.time() - t0
    d_recs, d_tiles = nat.DeviceBuffer.from_host(recs), nat.DeviceBuffer.from_host(tiles)
    cap = 8 * n + 1024
    d_pairs, d_total = nat.DeviceBuffer(cap * 8), nat.DeviceBuffer(8)
    e0, e1 = C.c_void_p(), C.c_void_p()
    nat.check(nat.lib().dcrx_event_create(C.byref(e0)))
    nat.check(nat.lib().dcrx_event_create(C.byref(e1)))
    L = nat.lib()
    nat.check(L.dcrx_umi_neighbours_device(d_recs.ptr, d_tiles.ptr, n_tiles, k, d_pairs.ptr, cap, d_total.ptr, None))   # warm-up
    nat.synchronize()
    times = []
    for _ in range(reps):
        nat.check(L.dcrx_event_record(e0, None))
        nat.check(L.dcrx_umi_neighbours_device(d_recs.ptr, d_tiles.ptr, n_tiles, k, d_pairs.ptr, cap, d_total.ptr, None))
        nat.check(L.dcrx_event_record(e1, None))
        nat.synchronize()
        ms = C.c_float()
        nat.check(L.dcrx_event_elapsed_ms(e0, e1, C.byref(ms)))
        times.append(ms.value)
    total = int(d_total.to_host(np.uint64, 1)[0])
    L.dcrx_event_destroy(e0)
    L.dcrx_event_destroy(e1)
    return min(times), total, encode_s


def synth_rows(n_rows, seed):
    """`.n12` rows: molecules of 1-4 reads each, 12-nt UMIs (M13 layout) with planted UMI errors, 60 DCRs."""
    rng = np.random.default_rng(seed)
    n_mol = max(1, n_rows // 2)
    umi = rng.integers(0, 4, size=(n_mol, 12), dtype=np.uint8)
    mol = np.sort(rng.integers(0, n_mol, size=n_rows))
    codes = umi[mol].copy()
    err = rng.random(n_rows) < 0.05
    pos = rng.integers(0, 12, size=n_rows)
    codes[err, pos[err]] = (codes[err, pos[err]] + 1) % 4
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].view("S12").ravel()
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n_mol, 32), dtype=np.uint8)].view("S32").ravel()
    dcr = rng.integers(0, 60, size=n_mol)
    lines = []
    for r in range(n_rows):
        b = bases[r].decode()
        m = int(mol[r])
        region = "GTCGTGACTGGGAAAACCCTGG" + b[:6] + "GTCGTGAT" + b[6:] + "ACGTAC"
        s = seqs[m].decode()
        lines.append(f"{dcr[m] % 40}, {dcr[m] % 12}, 1, 2, AC, r{r}, {s}, {'I' * 32}, {region}, {'I' * len(region)}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    out = {"metric": "collapse_stage2", "k": a.k, "kernel": [], "device": nat.device_name()}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        text, off = synth_umis(n, seed=n)
        ms, pairs, enc = kernel_ms(text, off, a.k)
        row = {"umis": len(off) - 1, "kernel_ms": round(ms, 3), "pairs": pairs, "host_encode_s": round(enc, 3)}
        if a.cpu_baseline and n <= 100000:
            sys.path.insert(0, ROOT)
            from tests import collapse_cluster_util as cu
            t0 = time.time()
            r, _ = cu.symdel_neighbours((text, off), a.k)
            row["cpu_baseline_symdel_1_thread_s"] = round(time.time() - t0, 2)
            row["cpu_baseline_pairs"] = len(r)
        out["kernel"].append(row)
    if a.rows:
        from decombinator_amd import collapse
        from decombinator_amd import io as dio
        with tempfile.TemporaryDirectory() as td:
            old = os.getcwd()
            os.chdir(td)
            try:
                open("dcr_BENCH_1_beta.n12", "w").write(synth_rows(a.rows, 7))
                inp = dio.cli_args(["collapse", "-in", "dcr_BENCH_1_beta.n12", "-c", "b", "--cluster", "-dz", "-dc", "-s"])
                t0 = time.time()
                sys.stdout, real = open(os.devnull, "w"), sys.stdout
                try:
                    rows = collapse.collapsinator(inp)
                    t1 = time.time()
                    from decombinator_amd.io import write_out_intermediate
                    write_out_intermediate(rows, inp, ".freq")
                finally:
                    sys.stdout.close()
                    sys.stdout = real
                t2 = time.time()
            finally:
                os.chdir(old)
        out["collapse"] = {"rows": a.rows, "total_s": round(t2 - t0, 3), "write_s": round(t2 - t1, 3), "freq_rows": len(rows),
                           **{k + "_s": round(v, 3) for k, v in collapse.stage_times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
