#!/usr/bin/env python3
"""The clonotype step (`--clonotypes`) on the GPU: one JSON line with, for random tables of 10^5, 10^6 and 4 * 10^6 entries
over a seeded coding gene set (tests/clonotype_util.coding_genes: 60 V x 13 J genes that code, two alleles of one gene):
  - the primitive dcrx_cdr3_device on device buffers (device events, median of --repeats after a warm-up), arena sized once;
  - the host entry dcrx_clonotypes (wall clock, with its copies in and out), median of --repeats after a warm-up;
  - the only baseline there is, on the same table and machine: dcrx_cdr3_batch (one host thread; the sizing call not
    counted) and a Python dict that groups its productive rows by (V call group, J call group, junction_aa).
The two sides' clonotype counts are compared.
Usage: tools/bench_clonotypes.py [--sizes 100000,1000000,4000000] [--repeats 5] [--no-baseline]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decombinator_amd import _native as nat  # noqa: E402
from decombinator_amd import translate  # noqa: E402
from tests import clonotype_util as cu  # noqa: E402


def random_table(G, n, seed, max_del=9, max_ins=7):
    """n random entries (not made distinct: the step takes any table), Zipf-like counts, count descending."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_ins + 1, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].tobytes()
    count = np.sort(np.maximum(1, (1000 / (1 + rng.pareto(1.2, n) * 20)).astype(np.uint64)))[::-1].copy()
    return {"v": rng.integers(0, len(G.v_regions), n).astype(np.int32), "j": rng.integers(0, len(G.j_regions), n).astype(np.int32),
            "vdel": rng.integers(0, max_del + 1, n).astype(np.int32), "jdel": rng.integers(0, max_del + 1, n).astype(np.int32),
            "count": count, "ins_off": off, "ins_text": text}


def time_device(genes, tab, repeats):
    n, text = len(tab["v"]), tab["ins_text"]
    d = [nat.DeviceBuffer.from_host(tab[k]) for k in ("v", "j", "vdel", "jdel", "ins_off")]
    d_text = nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))
    d_rows = nat.DeviceBuffer(n * nat.CLONO_ROW_DTYPE.itemsize)
    wb = nat.clono_work_bytes(n, len(text))
    d_work, d_need = nat.DeviceBuffer(wb), nat.DeviceBuffer(16)
    nat.cdr3_device(genes, n, *d, d_text, len(text), d_rows, None, 0, d_need, d_work, wb)
    nat.check(nat.lib().dcrx_synchronize())
    need = int(d_need.to_host(np.uint64, 1)[0])
    d_arena = nat.DeviceBuffer(max(16, need))
    e0, e1 = nat.Event(), nat.Event()
    ms = []
    for k in range(repeats + 1):
        e0.record()
        nat.cdr3_device(genes, n, *d, d_text, len(text), d_rows, d_arena, need, d_need, d_work, wb)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return {"cdr3_device_ms": round(statistics.median(ms), 3), "cdr3_device_ms_all": [round(x, 3) for x in ms], "arena_bytes": need}


def time_host_entry(genes, tab, repeats):
    wall = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        table, stats, _ = nat.clonotypes(genes, tab)
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"clonotypes_ms": round(statistics.median(wall), 2), "clonotypes_ms_all": [round(x, 2) for x in wall], "stats": stats}


def time_baseline(G, tab):
    n = len(tab["v"])
    g = translate._native_genes(G)
    rows = np.zeros(n, dtype=nat.CDR3_ROW_DTYPE)
    itext = np.frombuffer(tab["ins_text"] + b"\0", np.uint8)
    args = (C.byref(g.c), n, tab["v"].ctypes.data, tab["j"].ctypes.data, tab["vdel"].ctypes.data, tab["jdel"].ctypes.data,
            itext.ctypes.data, tab["ins_off"].ctypes.data, rows.ctypes.data)
    need = nat.check(int(nat.lib().dcrx_cdr3_batch(*args, None, 0)))
    text = np.empty(max(1, need), np.uint8)
    t0 = time.perf_counter()
    nat.check(int(nat.lib().dcrx_cdr3_batch(*args, text.ctypes.data, need)))
    batch_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    vg, jg = nat.call_groups(G.v_names), nat.call_groups(G.j_names)
    buf = text.tobytes()
    groups = {}
    for k in np.nonzero((rows["status"] == 0) & (rows["productive"] == 1))[0].tolist():
        r = rows[k]
        a = int(r["aa_off"]) + int(r["junction_aa_off"])
        key = (int(vg[tab["v"][k]]), int(jg[tab["j"][k]]), buf[a:a + int(r["junction_aa_len"])])
        groups[key] = groups.get(key, 0) + int(tab["count"][k])
    dict_ms = (time.perf_counter() - t0) * 1e3
    return {"cdr3_batch_ms": round(batch_ms, 1), "python_dict_grouping_ms": round(dict_ms, 1), "text_bytes": need, "clonotypes": len(groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    G = cu.coding_genes(3, n_v=60, n_j=13)
    genes = translate._clono_genes(G)
    res = {"device": nat.device_name(), "genes": "coding_genes(3, 60, 13)", "repeats": a.repeats, "tables": {}}
    for n in (int(x) for x in a.sizes.split(",")):
        tab = random_table(G, n, seed=n)
        r = {"entries": n}
        r.update(time_device(genes, tab, a.repeats))
        r.update(time_host_entry(genes, tab, a.repeats))
        if not a.no_baseline:
            r["baseline"] = time_baseline(G, tab)
            r["same_clonotype_count"] = r["baseline"]["clonotypes"] == r["stats"]["clonotypes_out"]
        res["tables"][str(n)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
