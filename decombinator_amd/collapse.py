"""Front half of the reference's `collapse` stage, per `.n12` row: spacer
search, UMI (barcode) extraction, barcode quality filter, inter-tag length filter — everything
`read_in_data` does to a row before it starts grouping rows (reference
src/decombinator/collapse.py:482-565, with get_barcode_positions :367-479, set_barcode :278-326,
check_umi_quality :343-353 and the spacer searches :192-236).  Grouping and clustering (the
stateful rest of the stage) are outside this build.

read_in_rows() / read_in_data() run the batch entry of the library (dcrx_collapse_front,
csrc/dcrx_collapse.cpp: threaded C++ over the row text libdcrx assembled): all three spacer searches
of the reference — verbatim, up to two substitutions, the indel form `{2i+2d+1s<=2}` (:198-201) — are
decided there, with the reference's counters.  The per-row functions the reference's tests call
(getOligo, spacerSearch, findFirstSpacer, findSecondSpacer, get_barcode_positions) keep their names,
arguments and counter keys and run on the same native code (dcrx_spacer_search, a one-row batch).
The reference's own `regex` patterns live in tests/collapse_regex_ref.py, as the differential checker.

The rest of the stage (`--cluster`; reference collapse.py:565-1226, DESIGN.md "Collapse, stage 2") keeps the reference's
function names: group_rows (the grouping half of read_in_data), create_clustering_objs, make_merge_groups (the UMI neighbour
search: _native.umi_neighbours, a HIP kernel), make_clusters (connected components in Python, as networkx's _plain_bfs
orders them), cluster_UMIs, write_clusters, collapsinate and collapsinator.  Grouping, the protoseq test of the edges and the
counting are libdcrx's host code (csrc/dcrx_collapse_back.cpp); the groups and clusters are handed round as lazy mappings
with the reference's keys and values, built only when a caller looks at them.
"""
from __future__ import annotations

import collections as coll
import collections.abc
import gzip
import os
import time

import numpy as np

counts = coll.Counter()

OLIGOS = {
    "m13": {"spcr1": "GTCGTGACTGGGAAAACCCTGG", "spcr2": "GTCGTGAT"},
    "i8": {"spcr1": "GTCGTGAT", "spcr2": "GTCGTGAT"},
    "i8_single": {"spcr1": "ATCACGAC"},
    "nebio": {"spcr1": "TACGGG"},
    "takara": {"spcr1": "GTACGGG"},
}


def getOligo(oligo_name):
    """collapse.py:174-189."""
    if oligo_name.lower() not in OLIGOS:
        print("Error: Failed to recognise oligo name. Please choose from " + str(list(OLIGOS.keys())))
        raise SystemExit
    return OLIGOS[oligo_name.lower()]


def spacerSearch(subseq, seq):
    """collapse.py:204-212: the matches of `subseq` in `seq`, verbatim, else with up to two substitutions, else with one inserted
    or deleted base — the strings regex.findall returns, found by libdcrx (dcrx_spacer_search)."""
    from . import _native as nat
    return [seq[a:a + n] for a, n in nat.spacer_search(seq, subseq)[0]]


def findFirstSpacer(oligo, seq, oligo_start, oligo_end):
    """collapse.py:215-219."""
    return spacerSearch(oligo["spcr1"], seq[oligo_start:oligo_end])


def findSecondSpacer(oligo, seq):
    """collapse.py:222-227."""
    return spacerSearch(oligo["spcr2"], seq[len(oligo["spcr1"]):])


def get_barcode_positions(bcseq, inputargs, counts):
    """collapse.py:367-479 for one barcode region: [b1start, b1end(, b2start, b2end)] or None, the reference's getbarcode_*
    keys bumped in `counts` — a one-row batch through dcrx_collapse_front."""
    from . import _native as nat
    name = str.lower(inputargs["oligo"])
    if name not in nat.COLLAPSE_OLIGOS:
        raise ValueError("The flag for the -ol input must be one of M13, I8, I8_single, NEBIO, or TAKARA.")
    if not bcseq.isascii() or "," in bcseq or "\n" in bcseq:
        raise ValueError("barcode region is not plain sequence text")
    row = ", ".join(["0", "0", "0", "0", "A", "id", "A", "I", bcseq, "I" * len(bcseq)]) + "\n"
    rows, _, cnt = nat.collapse_front(row.encode("ascii"), name, inputargs["allowNs"], 1 << 30, [0, len(bcseq) + 1, 0], n_threads=1)
    for key, v in zip(nat.COLLAPSE_COUNTERS, cnt.tolist()):
        if v and key.startswith("getbarcode_"):
            counts[key] += int(v)
    r = rows[0]
    if r["b1start"] < 0 and r["b1end"] < 0:
        return None
    locs = [int(r["b1start"]), int(r["b1end"])]
    return locs if name in ("nebio", "takara") else locs + [int(r["b2start"]), int(r["b2end"])]


def _rows_text(data) -> bytes:
    """The rows as `.n12` text (fields joined by ", ", one row per line): what libdcrx's batch entry reads."""
    chunks = getattr(data, "_tagged_chunks", None)
    if chunks is not None:                                   # the rows decombinator() returned: already text
        return b"".join(blob for _, blob, _ in chunks())
    out = []
    for line in data:
        if isinstance(line, (bytes, bytearray)):
            line = line.decode("utf-8", "replace")
        out.append(line.rstrip("\n") if isinstance(line, str) else ", ".join(str(x) for x in line))
    return ("\n".join(out) + ("\n" if out else "")).encode("utf-8")


class FrontRows(coll.abc.Sequence):
    """What the front half leaves of each input row, in input order: None for a dropped row, else
    (barcode, barcode_qualstring, dcr, seq, seq_qualstring, seq_id) — built from the library's per-row records and the row
    text only when asked for (a run has millions of rows; `status`, `barcode` and `kept()` give the columns at once)."""

    def __init__(self, text, rows, offsets, decided):
        self._text, self._rows, self._off, self._decided = text, rows, offsets, decided       # decided: {row index: entry} of the rows the regex path settled
        self.status = rows["status"]

    def __len__(self):
        return len(self._rows)

    def __eq__(self, other):
        if isinstance(other, (list, FrontRows)):
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        return NotImplemented

    def kept(self):
        """Indices of the rows that passed."""
        import numpy as np
        ok = self._rows["status"] == 0
        for k, v in self._decided.items():
            ok[k] = v is not None
        return np.nonzero(ok)[0]

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        if k in self._decided:
            return self._decided[k]
        r = self._rows[k]
        if r["status"] != 0:
            return None
        line = self._text[int(self._off[k]):int(self._off[k + 1])].decode("utf-8", "replace").rstrip("\n").split(", ")
        return (r["barcode"][:r["barcode_len"]].decode("ascii"), r["barcode_qual"][:r["barcode_qual_len"]].decode("ascii"),
                line[:5], line[6], line[7], line[5])


def read_in_rows(data, inputargs, barcode_quality_parameters, n_threads: int = 0):
    """What read_in_data (collapse.py:482-565) does to each row before grouping, over a whole batch.  `data`: the rows
    decombinator() returned (N12Rows), lists of fields, or `.n12` lines.  Returns a FrontRows (one entry per input row:
    None for a dropped row, else (barcode, barcode_qualstring, dcr, seq, seq_qualstring, seq_id)); the module's `counts`
    receives the reference's keys."""
    from . import _native as nat
    name = str.lower(inputargs["oligo"])
    if name not in nat.COLLAPSE_OLIGOS:
        raise ValueError("The flag for the -ol input must be one of M13, I8, I8_single, NEBIO, or TAKARA.")
    text = _rows_text(data)
    rows, offs, cnt = nat.collapse_front(text, name, inputargs["allowNs"], inputargs["lenthreshold"], barcode_quality_parameters,
                                         n_threads=n_threads)
    for key, v in zip(nat.COLLAPSE_COUNTERS, cnt.tolist()):
        if v:
            counts[key] += int(v)
    import numpy as np
    bad = np.nonzero(rows["status"] == nat.CF_DEFER)[0]
    if len(bad):      # not ten fields of ASCII text: the reference would fail on such a row too (an IndexError / a wrong column)
        k = int(bad[0])
        raise ValueError(f"row {k} is not a ten-field ASCII `.n12` row: " + text[int(offs[k]):int(offs[k + 1])].decode("utf-8", "replace")[:200])
    return FrontRows(text, rows, offs, {})


def read_in_data(data, inputargs, barcode_quality_parameters, lev_threshold_fraction=None, dont_count=True, opener=None):
    """The reference's entry (collapse.py:482-565) as far as this build goes: the rows' front half.  With
    inputargs["command"] == "collapse", `data` is the path of an `.n12` file (opened with `opener`, as the reference does);
    otherwise the rows decombinator() returned.  lev_threshold_fraction and the grouping it steers are outside this build."""
    if inputargs.get("command") == "collapse":
        fh = (opener or open)(data, "rt")
        try:
            data = fh.read().splitlines()
        finally:
            fh.close()
    if not data:
        raise ValueError("No reads found in input file. Check .n12 and log files for errors.")       # :508-511
    if not dont_count:
        print("Reading data in...")
    return read_in_rows(data, inputargs, barcode_quality_parameters)


# ---- stage 2: grouping, UMI clustering, counting (reference collapse.py:565-1226) -------------------------------------

stage_times = {}        # seconds per step of the last collapsinator call (tools/bench_collapse.py reads it)


def _dcretc(front, k, sampling):
    """The reference's dcretc of row k (collapse.py:567-590): "|".join([str(dcr), seq, seq_qualstring, seq_id]), plus barcode,
    barcode_qualstring, full barcode region and v_tail with -sa."""
    bc, bcq, dcr, seq, qual, sid = front[k]
    parts = [str(list(dcr)), seq, qual, sid]
    if sampling:
        f = front._text[int(front._off[k]):int(front._off[k + 1])].decode("utf-8", "replace").rstrip("\n").split(", ")
        parts += [bc, bcq, f[8], f[10]]
    return "|".join(parts)


class GroupedRows:
    """read_in_data's barcode_dcretc (collapse.py:585-683), backed by libdcrx's groups (dcrx_collapse_group): iterating gives
    the keys "barcode|0|protoseq" in the reference's dict order; members(g) builds group g's dcretc list when asked for."""

    def __init__(self, groups, front, sampling):
        self.groups, self.front, self.sampling = groups, front, sampling

    def __len__(self):
        return self.groups.n_groups

    def __iter__(self):
        return (self.key(g) for g in range(len(self)))

    def key(self, g):
        return self.groups.umi(g) + "|0|" + self.groups.protoseq(g)

    def members(self, g):
        mo, mr = self.groups.member_off, self.groups.member_rows
        return [_dcretc(self.front, int(r), self.sampling) for r in mr[int(mo[g]):int(mo[g + 1])]]


class _PerGroup(coll.abc.Sequence):
    """create_clustering_objs' lists over a GroupedRows: item(grouped, g) per group, in group order."""

    def __init__(self, grouped, item):
        self.grouped, self._item = grouped, item

    def __len__(self):
        return len(self.grouped)

    def __getitem__(self, g):
        return self._item(self.grouped, range(len(self))[g])


class Matches:
    """What make_merge_groups returns (a scipy coo_matrix in the reference): the pairs (row[e], col[e]), row < col, ascending."""

    def __init__(self, row, col, n):
        self.row, self.col, self.shape = row, col, (n, n)

    def getnnz(self):
        return len(self.row)


def group_rows(front, inputargs, lev_threshold_fraction):
    """The grouping half of read_in_data (collapse.py:585-683) over a FrontRows: a GroupedRows; `counts` receives
    readdata_barcode_dcretc_keys, number_input_unique_dcrs, number_input_total_dcrs, multi_tcr_barcodes and
    multi_tcr_barcode_reads.  (The reference's `ratio < 0.01 and > 3600 s` break, :526, is a wall-clock quirk: not
    reproduced, every row is read.)"""
    from . import _native as nat
    sampling = bool(inputargs.get("sampling_analysis"))
    groups = nat.Groups(front._text, front._off, front._rows, ", ", lev_threshold_fraction, sampling)
    for key, v in groups.counters.items():
        if key == "multi_tcr_barcode_reads":
            counts[key] += v
        else:
            counts[key] = v
    return GroupedRows(groups, front, sampling)


def create_clustering_objs(barcode_dcretc):
    """collapse.py:703-720 over a GroupedRows: (number of groups, [(key, dcretc list)], [(UMI, protoseq)])."""
    g = barcode_dcretc
    return (len(g), _PerGroup(g, lambda gr, k: (gr.key(k), gr.members(k))),
            _PerGroup(g, lambda gr, k: (gr.groups.umi(k), gr.groups.protoseq(k))))


def make_merge_groups(umi_protoseq_tuple, barcode_threshold, dont_count):
    """collapse.py:723-751: every pair of UMIs within Levenshtein distance barcode_threshold, (i, j) with i < j ascending —
    the UMI neighbour search of _native.umi_neighbours (dcrx_umi.hip on the GPU)."""
    from . import _native as nat
    g = umi_protoseq_tuple.grouped.groups
    n = len(umi_protoseq_tuple)
    if n == 0:
        raise ValueError("No UMIs to cluster, check .n12 file for errors")
    print("Clustering UMIs...")
    print("  ", n, "unique UMIs")
    row, col = nat.umi_neighbours((g.umi_text, g.umi_off), int(barcode_threshold))
    print("  ", len(row), "UMIs within edit distance of", barcode_threshold)
    return Matches(np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), n)


def _components(rows, cols):
    """networkx.connected_components on the graph of these edges, in its order (collapse.py:781): nodes in order of first
    appearance in the edges, each node's neighbours in edge order, a BFS per unseen node into a Python set (`_plain_bfs`) —
    each component's list(set) order is CPython's set order, which names the cluster and orders its members."""
    adj = {}
    for i, j in zip(rows, cols):
        adj.setdefault(i, []).append(j)
        adj.setdefault(j, []).append(i)
    n = len(adj)
    seen_all = set()
    out = []
    for v in adj:
        if v in seen_all:
            continue
        seen = {v}
        nextlevel = [v]
        while nextlevel:
            thislevel, nextlevel = nextlevel, []
            for u in thislevel:
                for w in adj[u]:
                    if w not in seen:
                        seen.add(w)
                        nextlevel.append(w)
                if len(seen) == n:
                    break
            if len(seen) == n:
                break
        seen_all.update(seen)
        out.append(list(seen))
    return out, adj


class Clusters:
    """make_clusters' result (collapse.py:754-809): iterating gives the keys (each cluster's base group key), values_of(c) the
    groups' dcretc lists concatenated; merged clusters first (components in networkx's order, members in list(set) order),
    then the groups in no edge, in group order.  cluster_groups / cluster_off hold the same as group indices."""

    def __init__(self, group_list, cluster_groups, cluster_off):
        self.group_list, self.cluster_groups, self.cluster_off = group_list, cluster_groups, cluster_off

    def __len__(self):
        return len(self.cluster_off) - 1

    def _groups(self, c):
        return self.cluster_groups[int(self.cluster_off[c]):int(self.cluster_off[c + 1])]

    def __iter__(self):
        return (self.group_list[int(self._groups(c)[0])][0] for c in range(len(self)))

    def values_of(self, c):
        out = []
        for g in self._groups(c):
            out += self.group_list[int(g)][1]
        return out


def make_clusters(merge_groups, barcode_dcretc_list, lev_threshold_fraction):
    """collapse.py:754-809: keep the edges whose two protoseqs are equivalent (libdcrx, threaded), then the components."""
    rows, cols = np.asarray(merge_groups.row, dtype=np.int64), np.asarray(merge_groups.col, dtype=np.int64)
    keep = barcode_dcretc_list.grouped.groups.equivalent(rows, cols, lev_threshold_fraction)
    rows, cols = rows[keep].tolist(), cols[keep].tolist()
    counts["n_merged_UMIs"] = len(rows)
    print("    ", len(rows), "merged UMIs")
    comps, adj = _components(rows, cols)
    n = len(barcode_dcretc_list)
    in_graph = np.zeros(n, dtype=bool)
    if adj:
        in_graph[np.fromiter(adj.keys(), dtype=np.int64, count=len(adj))] = True
    lone = np.nonzero(~in_graph)[0]
    sizes = [len(c) for c in comps]
    cluster_groups = np.empty(sum(sizes) + len(lone), dtype=np.uint32)
    cluster_groups[:sum(sizes)] = [g for c in comps for g in c]
    cluster_groups[sum(sizes):] = lone
    cluster_off = np.zeros(len(comps) + len(lone) + 1, dtype=np.uint64)
    cluster_off[1:] = np.cumsum(np.concatenate([np.asarray(sizes, dtype=np.uint64), np.ones(len(lone), dtype=np.uint64)]))
    return Clusters(barcode_dcretc_list, cluster_groups, cluster_off)


def _unique_name(filename, ftype):
    count = 1
    while os.path.isfile(filename + ftype):
        filename = filename + str(count)
        count += 1
    return filename + ftype


def write_clusters(clusters, inputargs, text):
    """collapse.py:813-843: clusters_<chain>[N].psv.gz in the working directory; `text`: the lines dcrx_collapse_count wrote."""
    from . import _native as nat
    filename = _unique_name("clusters_" + inputargs["chain"], ".psv.gz")
    print("   Writing clusters to directory: ", os.path.abspath(filename), "...")
    header_names = ["umi_id", "dcr", "inter_tag", "inter_tag_qual", "read_id", "umi", "umi_qual", "full_oligo", "v_tail"]
    with nat.GzipWriter(filename, level=9) as gz:
        gz.write(("|".join(header_names) + "\n").encode())
        gz.write(text)
    return filename


def cluster_UMIs(barcode_dcretc, inputargs, barcode_threshold, lev_threshold_fraction, dont_count):
    """collapse.py:846-894: the groups merged into clusters (a Clusters)."""
    print("Clustering barcode groups...")
    t0 = time.time()
    num_initial_groups, barcode_dcretc_list, umi_protoseq_tuple = create_clustering_objs(barcode_dcretc)
    matches = make_merge_groups(umi_protoseq_tuple, barcode_threshold, dont_count)
    t1 = time.time()
    print("  ", "comparing TCR sequences of similar UMIs...")
    clusters = make_clusters(matches, barcode_dcretc_list, lev_threshold_fraction)
    t2 = time.time()
    stage_times["neighbours"], stage_times["graph"] = t1 - t0, t2 - t1
    print("  ", num_initial_groups, "groups merged into", len(clusters), "clusters")
    print("  ", round(t2 - t0, 10), "seconds")
    return clusters


class FreqRows(coll.abc.Sequence):
    """collapsinate's out_data: one [v, j, vdel, jdel, insert, count, round(mean cluster size)] per DCR (the first five as
    the `.n12` strings), held as the `.freq` text libdcrx wrote; write_text() hands that text on as it is."""

    def __init__(self, text: bytes):
        self.text = text
        self._lines = None

    def _rows(self):
        if self._lines is None:
            self._lines = self.text.decode("utf-8").splitlines()
        return self._lines

    def __len__(self):
        return self.text.count(b"\n")

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        f = self._rows()[k].split(", ")
        return f[:5] + [int(f[5]), int(f[6])]

    def write_text(self, fh, joiner=", "):
        if joiner != ", ":
            raise ValueError("FreqRows are written with the `.freq` separator only")
        fh.write(self.text.decode("utf-8"))


def collapsinate(data, inputargs, barcode_quality_parameters, lev_threshold_fraction, barcode_distance_threshold, outpath, file_id,
                 dont_count, opener=None):
    """collapse.py:897-977: (out_data, collapsed, average_cluster_size_counter)."""
    from statistics import median
    t0 = time.time()
    if inputargs.get("command") == "collapse":
        fh = (opener or open)(data, "rt")
        try:
            data = fh.read().splitlines()
        finally:
            fh.close()
    if not data:
        raise ValueError("No reads found in input file. Check .n12 and log files for errors.")
    print("Reading data in...")
    front = read_in_rows(data, inputargs, barcode_quality_parameters)
    t1 = time.time()
    barcode_dcretc = group_rows(front, inputargs, lev_threshold_fraction)
    t2 = time.time()
    stage_times["front"], stage_times["grouping"] = t1 - t0, t2 - t1
    print("   Read in total of", counts["readdata_input_dcrs"], "lines")
    print("  ", counts["readdata_success"], "reads sorted into", len(barcode_dcretc), "initial groups")
    clusters = cluster_UMIs(barcode_dcretc, inputargs, barcode_distance_threshold, lev_threshold_fraction, dont_count)
    print("Collapsing clusters...")
    t3 = time.time()
    extra = bool(inputargs.get("writeclusters") or inputargs.get("barcodeduplication"))
    votes, size_sum, freq, wc, bd = barcode_dcretc.groups.count(clusters.cluster_groups, clusters.cluster_off, extra)
    out_data = FreqRows(freq)
    av = np.rint(size_sum.astype(np.float64) / np.maximum(votes, 1).astype(np.float64)).astype(np.int64)
    counts["number_output_unique_dcrs"] = len(votes)
    counts["number_output_total_dcrs"] = int(votes.sum())
    counts["median_barcodes_per_tcr"] = float(median(votes.tolist()))
    average_cluster_size_counter = coll.Counter(av.tolist())
    t4 = time.time()
    stage_times["counting"] = t4 - t3
    if inputargs.get("writeclusters"):
        write_clusters(clusters, inputargs, wc)
    if inputargs.get("barcodeduplication"):
        outfile = outpath + file_id + "_barcode_duplication.txt"
        with open(outfile, "w") as outhandle:
            outhandle.write(bd.decode("utf-8"))
        print("barcode duplication data saved to", outfile)
    stage_times["extra_writes"] = time.time() - t4
    counts["outfilenam"] = "Saved to variable"
    collapsed = coll.Counter({str(r[:5]): r[5] for r in out_data})
    return out_data, collapsed, average_cluster_size_counter


def _summary_body(inputargs, n):
    """The counters' part of the Collapsing_Summary.csv (collapse.py:1110-1184), after the Version / Directory / file / date
    lines."""
    s = ""
    for key in ["extension", "dontgzip", "allowNs", "dontcheckinput", "barcodeduplication", "minbcQ", "bcQbelowmin", "bcthreshold",
                "lenthreshold", "percentlevdist", "avgQthreshold", "positionalbarcodes", "oligo"]:
        s += key + "," + str(inputargs[key]) + "\n"
    n["pc_input_dcrs"] = n["number_input_total_dcrs"] / n["readdata_input_dcrs"]
    n["pc_uniq_dcr_kept"] = n["number_output_unique_dcrs"] / n["number_input_unique_dcrs"]
    n["pc_total_dcr_kept"] = n["number_output_total_dcrs"] / n["number_input_total_dcrs"]
    n["avg_input_tcr_size"] = n["number_input_total_dcrs"] / n["number_input_unique_dcrs"]
    n["avg_output_tcr_size"] = n["number_output_total_dcrs"] / n["number_output_unique_dcrs"]
    n["avg_RNA_duplication"] = 1 / n["pc_total_dcr_kept"]
    return (s + "\nInputUncollapsedDCRLines," + str(n["readdata_input_dcrs"])
            + "\nUniqueDCRsPassingFilters," + str(n["number_input_unique_dcrs"])
            + "\nTotalDCRsPassingFilters," + str(n["number_input_total_dcrs"])
            + "\nPercentDCRPassingFilters(withbarcode)," + str(round(n["pc_input_dcrs"], 3))
            + "\nUniqueDCRsPostCollapsing," + str(n["number_output_unique_dcrs"])
            + "\nTotalDCRsPostCollapsing," + str(n["number_output_total_dcrs"])
            + "\nPercentUniqueDCRsKept," + str(round(n["pc_uniq_dcr_kept"], 3))
            + "\nPercentTotalDCRsKept," + str(round(n["pc_total_dcr_kept"], 3))
            + "\nAverageInputTCRAbundance," + str(round(n["avg_input_tcr_size"], 3))
            + "\nAverageOutputTCRAbundance," + str(round(n["avg_output_tcr_size"], 3))
            + "\nAverageRNAduplication," + str(round(n["avg_RNA_duplication"], 3))
            + "\n\nBarcodeFail_ContainedNs," + str(n["getbarcode_fail_N"])
            + "\nBarcodeFail_SpacersNotFound," + str(n["readdata_fail_no_bclocs"])
            + "\nBarcodeFail_LowQuality," + str(n["readdata_fail_low_barcode_quality"])
            + "\nNumberMultiTCRBarcodes," + str(n["multi_tcr_barcodes"])
            + "\nNumberMultiTCRBarcodeReads," + str(n["multi_tcr_barcode_reads"])
            + "\nMedianUMIsPerTCR," + str(n["median_barcodes_per_tcr"]))


def collapsinator(inputargs: dict, data=None):
    """collapse.py:980-1226: the whole stage over inputargs["infile"] (command "collapse") or the rows decombinator()
    returned; writes the Collapsing_Summary.csv (unless -s) and the -uh / -bd / -wc files; returns the `.freq` rows (a
    FreqRows)."""
    from .decombine import __version__
    print("Running Collapsinator (MI355X / HIP build) version", __version__)
    if inputargs.get("extension", "n12") == "n12":
        inputargs["extension"] = "freq"
    opener = gzip.open if inputargs["infile"].endswith(".gz") else open
    counts.clear()
    stage_times.clear()
    start = time.time()
    barcode_quality_parameters = [inputargs["minbcQ"], inputargs["bcQbelowmin"], inputargs["avgQthreshold"]]
    lev_threshold_fraction = inputargs["percentlevdist"] / 100
    if inputargs["command"] == "collapse":
        data = inputargs["infile"]
    file_id = inputargs["infile"].split("/")[-1].split(".")[0]
    out_data, collapsed, average_cluster_size_counter = collapsinate(
        data, inputargs, barcode_quality_parameters, lev_threshold_fraction, inputargs["bcthreshold"], "", file_id,
        inputargs["dontcount"], opener)
    taken = time.time() - start
    chainnams = {"a": "alpha", "b": "beta", "g": "gamma", "d": "delta"}
    chain = inputargs["chain"]
    if not inputargs["suppresssummary"]:
        logpath = inputargs["outpath"] + f"Logs{os.sep}"
        sample_name = file_id.split(os.sep)[-1]
        os.makedirs(logpath, exist_ok=True)
        date = time.strftime("%Y_%m_%d")
        stem = logpath + date + "_" + "dcr_" + sample_name + f"_{chainnams[chain.lower()]}" + "_Collapsing_Summary"
        summaryname = stem + ".csv"
        if os.path.exists(summaryname):
            for i in range(2, 10000):
                summaryname = stem + str(i) + ".csv"
                if not os.path.exists(summaryname):
                    break
        inout_name = "_".join(f"{file_id}".split("_")[:-1]) + f"_{chainnams[chain.lower()]}"
        head = ("Property,Value\nVersion," + __version__ + "\nDirectory," + os.getcwd() + "\nInputFile," + inout_name
                + "\nOutputFile," + inout_name + "\nDateFinished," + date + "\nTimeFinished," + time.strftime("%H:%M:%S")
                + "\nTimeTaken(Seconds)," + str(round(taken, 2)) + "\n\n")
        with open(summaryname, "w") as summaryfile:
            print(head + _summary_body(inputargs, counts), file=summaryfile)
        if inputargs["UMIhistogram"]:
            hfileprefix = "_".join(summaryname.split("_")[:-2] + ["UMIhistogram"])
            if os.path.exists(hfileprefix + ".csv"):
                i = 1
                while os.path.exists(hfileprefix + str(i) + ".csv"):
                    i += 1
                hfileprefix += str(i)
            hfilename = hfileprefix + ".csv"
            with open(hfilename, "w") as hfile:
                for av, count in sorted(average_cluster_size_counter.items()):
                    print(str(av) + "," + str(count), file=hfile)
            print("\nAverage UMI cluster size histogram data saved to", hfilename)
    return out_data
