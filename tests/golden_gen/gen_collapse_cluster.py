#!/usr/bin/env python3
"""Generates tests/golden/collapse_cluster.json: the reference's UNMODIFIED collapse.py (its collapsinator, the whole of stage 2:
grouping, UMI clustering, counting) over synthetic `.n12` rows with planted UMI families.  Run on a development machine that
has the reference's sources (REFERENCE_SRC, default /root/reference/src) — never by a test.

Stand-ins for the wheels that are absent offline: polyleven from oracle/refshim (read-only), and this directory's pyrepseq
(a brute-force symdel: every pair within the distance, decided by that polyleven).  networkx, scipy and regex are the real
ones.  The rows come from tests/collapse_cluster_util.synth_rows (seeded; the tests make the same rows).  Per case: the
parameters, the `.freq` lines in order, the reference's counters, the Collapsing_Summary body (from the blank line after
TimeTaken on: no date, directory or version) and, for one case, the -uh output and the SHA-256 of the -bd and -wc outputs.  The generator asserts that every case covers multi-TCR barcodes, protoseq re-keys, ties in both
most_common calls, components of five or more nodes whose list(set) order is not sorted, and means of exactly .5."""
import collections as coll
import gzip
import hashlib
import importlib.metadata
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "oracle", "refshim"), os.environ.get("REFERENCE_SRC", "/root/reference/src")]
_v = importlib.metadata.version
importlib.metadata.version = lambda n: "0" if n == "decombinator" else _v(n)
import networkx as nx  # noqa: E402
from decombinator import collapse as ref  # noqa: E402
from tests.collapse_cluster_util import synth_rows  # noqa: E402

class Capture:
    def __init__(self):
        self.barcode_dcretc = None
        self.components = []
        self.clusters = None


def run_case(params, rows, extra):
    cap = Capture()
    orig_read, orig_cluster = ref.read_in_data, ref.cluster_UMIs
    ref.read_in_data = lambda *a, **k: setattr(cap, "barcode_dcretc", orig_read(*a, **k)) or cap.barcode_dcretc
    ref.cluster_UMIs = lambda *a, **k: setattr(cap, "clusters", orig_cluster(*a, **k)) or cap.clusters

    def comps(G):
        for c in nx.connected_components(G):
            cap.components.append(list(c))
            yield c

    ref.nx = types.SimpleNamespace(Graph=nx.Graph, connected_components=comps)
    counts_seen = {}
    orig_collapsinate = ref.collapsinate

    def collapsinate(*a, **k):
        out = orig_collapsinate(*a, **k)
        counts_seen.update(ref.counts)
        return out

    ref.collapsinate = collapsinate
    old = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            with open("dcr_CASE_1_beta.n12", "w") as fh:
                fh.write("\n".join(rows) + "\n")
            args = dict(infile="dcr_CASE_1_beta.n12", command="collapse", chain="b", extension="n12", suppresssummary=False,
                        dontgzip=True, dontcount=True, outpath="", allowNs=params["allowNs"], dontcheckinput=True,
                        barcodeduplication=extra, positionalbarcodes=False, minbcQ=20, bcQbelowmin=1, avgQthreshold=30,
                        bcthreshold=params["bcthreshold"], lenthreshold=130, percentlevdist=params["percentlevdist"],
                        oligo=params["oligo"], writeclusters=extra, UMIhistogram=extra, sampling_analysis=False)
            out = ref.collapsinator(args)
            logs = sorted(os.listdir("Logs"))
            summ = open(os.path.join("Logs", [x for x in logs if "Collapsing_Summary" in x][0])).read()
            res = {"freq": [", ".join(map(str, r)) for r in out],
                   "summary_body": summ.split("\n\n", 1)[1],
                   "counts": {k: (float(v) if isinstance(v, float) else v) for k, v in counts_seen.items()
                              if not k.startswith("time") and k not in ("start_time", "end_time", "outfilenam")}}
            if extra:
                res["bd_sha256"] = hashlib.sha256(open("dcr_CASE_1_beta_barcode_duplication.txt", "rb").read()).hexdigest()
                res["uh"] = open(os.path.join("Logs", [x for x in logs if "UMIhistogram" in x][0])).read()
                res["wc_sha256"] = hashlib.sha256(gzip.open("clusters_b.psv.gz", "rb").read()).hexdigest()
        finally:
            os.chdir(old)
            ref.read_in_data, ref.cluster_UMIs, ref.collapsinate, ref.nx = orig_read, orig_cluster, orig_collapsinate, nx
    return res, cap


def coverage(cap, counts):
    """How often the case exercises each corner of the contract."""
    cov = coll.Counter()
    cov["multi_tcr_barcodes"] = counts["multi_tcr_barcodes"]
    for key, lst in cap.barcode_dcretc.items():
        seqs = [x.split("|")[1] for x in lst]
        if seqs[0] != key.split("|")[2]:
            cov["rekeys"] += 1
        mc = coll.Counter(seqs).most_common(2)
        if len(mc) == 2 and mc[0][1] == mc[1][1]:
            cov["seq_ties"] += 1
    sizes = coll.defaultdict(list)
    for key, lst in cap.clusters.items():
        mc = coll.Counter(x.split("|")[0] for x in lst).most_common(2)
        if len(mc) == 2 and mc[0][1] == mc[1][1]:
            cov["dcr_ties"] += 1
        sizes[mc[0][0]].append(len(lst))
    for c in cap.components:
        if len(c) >= 5 and c != sorted(c):
            cov["unsorted_components_ge5"] += 1
    for s in sizes.values():
        if (2 * sum(s)) % len(s) == 0 and (sum(s) * 2 // len(s)) % 2 == 1:
            cov["half_means"] += 1
    return cov


def main():
    cases = [
        dict(name="m13_bc1_lv10_N", oligo="M13", bcthreshold=1, percentlevdist=10, allowNs=True, seed=11, n_rows=4000),
        dict(name="m13_bc2_lv20", oligo="M13", bcthreshold=2, percentlevdist=20, allowNs=False, seed=12, n_rows=4000),
        dict(name="m13_bc3_lv10", oligo="M13", bcthreshold=3, percentlevdist=10, allowNs=False, seed=13, n_rows=4000),
        dict(name="i8_single_bc2_lv10_extra", oligo="I8_single", bcthreshold=2, percentlevdist=10, allowNs=False, seed=14, n_rows=4000),
    ]
    out = {"generator": "tests/golden_gen/gen_collapse_cluster.py", "cases": []}
    for c in cases:
        rows = synth_rows(c["seed"], c["oligo"].lower(), c["n_rows"], c["allowNs"])
        extra = c["name"].endswith("extra")
        res, cap = run_case(c, rows, extra)
        cov = coverage(cap, res["counts"])
        print(c["name"], len(res["freq"]), "freq rows;", dict(cov))
        for k in ("multi_tcr_barcodes", "rekeys", "seq_ties", "dcr_ties", "unsorted_components_ge5", "half_means"):
            assert cov[k] >= 3, (c["name"], k, cov[k])
        out["cases"].append(dict(params={k: c[k] for k in ("name", "oligo", "bcthreshold", "percentlevdist", "allowNs", "seed", "n_rows")},
                                 extra=extra, coverage=dict(cov), **res))
    path = os.path.join(ROOT, "tests", "golden", "collapse_cluster.json")
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
