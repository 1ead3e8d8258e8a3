#!/usr/bin/env python3
"""`motifs --groups` on the GPU: one JSON line with, for seeded tables of 10^4, 10^5 and 10^6 units (strings of 11 to 18 random
residues, every fourth one a one-residue copy of another so that the distance links something), K = {2,3,4}, trim 3,3, S = 10^2
and 10^4 selected motifs and G = 0 and 1:
  - members: dcrx_cdr3_motif_members_device on device buffers (device events) — the counting call, then the call that writes
    exactly `need` members —, median of --repeats after a warm-up, beside the one baseline there is on a GPU: `motifs` at
    R = 0 on the same units (dcrx_cdr3_motifs_device with no background), the same walk over the units without the write;
  - neighbours (G > 0): dcrx_cdr3_neighbours_device, the degree pass and the call that writes the adjacency;
  - components: dcrx_cdr3_groups_device on the members and the adjacency (device events around the call, its one wait per
    round inside), and the number of rounds;
  - the host entry dcrx_cdr3_motif_groups as the stage calls it (wall clock, with its copies in and out).
The selected motifs are taken from the units themselves: of the motifs at least three units hold, in order of how many hold
them, S at even steps — so the list runs from the 2-mers a tenth of the table holds to 4-mers three units hold.
Beside the Python contract on one thread (tests/motif_groups_util.expected_groups: every pair of units compared) at --python-units
(default 10^4) and S = 10^2, G = 1; both sides must agree.  --out FILE rewrites the result so far after every table.
Usage: tools/bench_cdr3_groups.py [--units 10000,100000,1000000] [--selected 100,10000] [--distances 0,1] [--repeats 3]
                                  [--no-python] [--python-units 10000] [--out FILE]"""
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
from tests import motif_groups_util as gu  # noqa: E402
from tests import motif_util as mu  # noqa: E402

KS, TRIM = (2, 3, 4), (3, 3)
WIDTH = 18


def seeded_units(count, seed):
    """(off, text) of `count` random units; unit 4 q + 1 is unit 4 q with one residue replaced (where both have one length)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(mu.AMINO, np.uint8)
    mat, lens = letters[rng.integers(0, len(letters), (count, WIDTH))], rng.integers(11, WIDTH + 1, count)
    src = np.arange(0, count - 1, 4)
    mat[src + 1], lens[src + 1] = mat[src], lens[src]
    at = rng.integers(0, 11, len(src))
    mat[src + 1, at] = letters[(np.searchsorted(letters, mat[src, at]) + rng.integers(1, 20, len(src))) % 20]
    off = np.zeros(count + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off, mat[np.arange(WIDTH)[None, :] < lens[:, None]].tobytes()


def selected_of(off, text, S):
    """S motifs of the units at even steps through those at least three units hold, most held first; in motif order."""
    empty = np.zeros(1, np.uint64)
    found = nat.cdr3_motifs(off, text, empty, b"", KS, TRIM, 3, 0, 1)
    order = np.argsort(-found["cs"].astype(np.int64), kind="stable")
    pick = np.sort(order[np.linspace(0, len(order) - 1, min(S, len(order))).astype(np.int64)])
    return found["k"][pick].astype(np.uint32), found["code"][pick].astype(np.uint32)


def median_ms(run, repeats):
    e0, e1, ms = nat.Event(), nat.Event(), []
    for k in range(repeats + 1):
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_ms(e1))
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def time_parts(off, text, sel_k, sel_code, G, repeats):
    n, S = len(off) - 1, len(sel_k)
    dev = nat.DeviceBuffer.from_host
    d_off, d_text, d_k, d_code = dev(off), dev(np.frombuffer(text, np.uint8)), dev(sel_k), dev(sel_code)
    d_nm, d_mo, d_need = nat.DeviceBuffer(4 * n), nat.DeviceBuffer(8 * (S + 1)), nat.DeviceBuffer(16)
    row = {}
    # members: the counting call, then exactly `need`
    wb0 = nat.cdr3_motif_members_work_bytes(n, 0)
    d_w0 = nat.DeviceBuffer(wb0)
    count = lambda: nat.cdr3_motif_members_device(n, d_off, d_text, KS, TRIM, S, d_k, d_code, 0, d_nm, d_mo, None, d_need, d_w0, wb0)
    row["members_count_ms"], row["members_count_ms_all"] = median_ms(count, repeats)
    need = int(d_need.to_host(np.uint64, 1)[0])
    wb = nat.cdr3_motif_members_work_bytes(n, need)
    d_w, d_mem = nat.DeviceBuffer(wb), nat.DeviceBuffer(4 * need + 16)
    write = lambda: nat.cdr3_motif_members_device(n, d_off, d_text, KS, TRIM, S, d_k, d_code, need, d_nm, d_mo, d_mem, d_need, d_w, wb)
    row["members_write_ms"], row["members_write_ms_all"] = median_ms(write, repeats)
    row.update(members_ms=round(row["members_count_ms"] + row["members_write_ms"], 3), members=need, members_work_bytes=wb)
    # the baseline: `motifs` at R = 0 on the same units, no background
    cap = min(n * 90, nat.CDR3_MOTIF_COUNT)
    wbm = nat.cdr3_motifs_work_bytes(n, 0, 0)
    d_out, d_st, d_wm = [nat.DeviceBuffer(8 * cap + 16) for _ in range(7)], nat.DeviceBuffer(ctypes.sizeof(nat.Cdr3MotifStatsC)), nat.DeviceBuffer(wbm)
    d_b_off = dev(np.zeros(1, np.uint64))
    counts = lambda: nat.cdr3_motifs_device(n, d_off, d_text, 0, d_b_off, d_text, KS, TRIM, 3, 0, 1, cap, *d_out, d_need, d_st, d_wm, wbm, None)
    row["motifs_r0_ms"], row["motifs_r0_ms_all"] = median_ms(counts, repeats)
    row["members_over_motifs_r0"] = round(row["members_ms"] / row["motifs_r0_ms"], 2)
    del d_out, d_wm
    # neighbours
    d_deg, d_adj_off, d_adj_need = nat.DeviceBuffer(4 * n), nat.DeviceBuffer(8 * (n + 1)), nat.DeviceBuffer(16)
    nat.check(nat.lib().dcrx_memset_device(d_adj_off.ptr, 0, 8 * (n + 1)))
    d_adj, adj_need = None, 0
    if G:
        d_cls = dev(np.zeros(n, np.uint32))
        wbn = nat.cdr3net_work_bytes(n, len(text))
        d_wn = nat.DeviceBuffer(wbn)
        degrees = lambda: nat.cdr3_neighbours_device(n, d_cls, d_off, d_text, len(text), G, d_deg, d_adj_off, None, 0, d_adj_need, d_wn, wbn)
        row["neighbours_degree_ms"], row["neighbours_degree_ms_all"] = median_ms(degrees, repeats)
        adj_need = int(d_adj_need.to_host(np.uint64, 1)[0])
        d_adj = nat.DeviceBuffer(4 * adj_need + 16)
        both = lambda: nat.cdr3_neighbours_device(n, d_cls, d_off, d_text, len(text), G, d_deg, d_adj_off, d_adj, adj_need, d_adj_need, d_wn, wbn)
        row["neighbours_write_ms"], row["neighbours_write_ms_all"] = median_ms(both, repeats)      # (the call runs the degree pass again)
        row.update(neighbours_ms=round(row["neighbours_degree_ms"] + row["neighbours_write_ms"], 3), adjacency=adj_need)
    # components
    wbg = nat.cdr3_groups_work_bytes(n, S)
    d_wg, d_w8 = nat.DeviceBuffer(wbg), dev(np.ones(n, np.uint64))
    d_of, d_head, d_units, d_wout, d_groups = (nat.DeviceBuffer(8 * n + 16) for _ in range(5))
    rounds = []
    groups = lambda: rounds.append(nat.cdr3_groups_device(n, d_w8, d_adj_off, d_adj if adj_need else None, adj_need, S, d_mo, d_mem if need else None,
                                                          need, d_of, d_head, d_units, d_wout, d_groups, d_wg, wbg))
    row["components_ms"], row["components_ms_all"] = median_ms(groups, repeats)
    row.update(rounds=rounds[-1], groups=int(d_groups.to_host(np.uint32, 1)[0]), components_work_bytes=wbg)
    return row


def time_host_entry(off, text, sel_k, sel_code, G, repeats):
    w, ms, out = np.ones(len(off) - 1, np.uint64), [], None
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        out = nat.cdr3_motif_groups(off, text, w, KS, TRIM, sel_k, sel_code, G, mem_cap=0)
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"host_entry_ms": round(statistics.median(ms), 2), "host_entry_ms_all": [round(x, 2) for x in ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--units", default="10000,100000,1000000")
    ap.add_argument("--selected", default="100,10000")
    ap.add_argument("--distances", default="0,1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--python-units", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"bench": "cdr3_groups", "device": nat.device_name(), "k": list(KS), "trim": list(TRIM), "tables": {}}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(result) + "\n")
    for i, n in enumerate(map(int, a.units.split(","))):
        off, text = seeded_units(n, 300 + i)
        for S in map(int, a.selected.split(",")):
            sel_k, sel_code = selected_of(off, text, S)
            for G in map(int, a.distances.split(",")):
                row = time_parts(off, text, sel_k, sel_code, G, a.repeats)
                got, host = time_host_entry(off, text, sel_k, sel_code, G, a.repeats)
                row.update(host, selected=len(sel_k), stats=got["stats"])
                assert got["stats"]["groups"] == row["groups"] and got["need"] == row["members"]
                result["tables"][f"n{n}_S{S}_G{G}"] = row
                save()
    if not a.no_python:
        n = a.python_units
        off, text = seeded_units(n, 300)
        sel_k, sel_code = selected_of(off, text, 100)
        units, w = gu.cut(off, text), [1] * n
        t0 = time.perf_counter()
        want = gu.expected_groups(units, w, KS, TRIM, list(zip(sel_k.tolist(), sel_code.tolist())), 1)
        seconds = time.perf_counter() - t0
        got, host = time_host_entry(off, text, sel_k, sel_code, 1, a.repeats)
        gu.assert_same(nat.cdr3_motif_groups(off, text, w, KS, TRIM, sel_k, sel_code, 1), want)
        result["python_one_thread"] = {"units": n, "selected": len(sel_k), "distance": 1, "seconds": round(seconds, 2),
                                       "host_entry_ms": host["host_entry_ms"], "agrees": True}
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
