"""Workloads on gene-family tag sets (oracle/family.py), shared by tests/test_family_tagsets.py (host emulation) and
tests/test_gpu_family_tagsets.py (the HIP path): built once per process, with the oracle's results beside them."""
from __future__ import annotations

import functools

import numpy as np

from decombinator_amd import _native as nat
from oracle import family
from oracle import oracle as orc
from tests import parity_util as pu

SEEDS = {"original": 1000, "extended": 3000}
FOUND_NOT = (4, 5, 9, 10)          # dcrx_status: a side's half-1 / half-2 hits exhausted (found...not...)


def tagset_dict(ts) -> dict:
    vs, js = ts.half_splits
    return dict(v_tags=ts.v_tags, v_jumps=ts.v_jumps, v_regions=ts.v_regions, j_tags=ts.j_tags, j_jumps=ts.j_jumps,
                j_regions=ts.j_regions, v_half_split=vs, j_half_split=js)


def oracle_tables(ts) -> orc.OracleTables:
    return orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                            [r.upper() for r in ts.j_regions], *ts.half_splits)


@functools.lru_cache(maxsize=None)
def tagset(split: str):
    """The two family sets of the tests: beta-like with the original split (10 + 10, 6 + 14), alpha-like with the
    extended one (10 + 10 both); 40 V and 12 J tags, related regions, decoys."""
    return family.make_family_tagset(31, "original", "b") if split == "original" else family.make_family_tagset(32, "extended", "a")


def strands(sense, orientation: str):
    """The reads as the batch holds them: `reverse` on the stored strand, `forward` on the sense strand, `both` on
    alternating strands."""
    if orientation == "forward":
        return list(sense)
    if orientation == "reverse":
        return [orc.revcomp(r) for r in sense]
    return [r if i % 2 else orc.revcomp(r) for i, r in enumerate(sense)]


class Workload:
    """Sense-frame reads of one tag set, their marks, and per (orientation, allow_ns) the batch's reads and the
    oracle's records and counters (computed on first use, then left alone)."""

    def __init__(self, ts, sense, marks):
        self.ts, self.sense, self.marks = ts, sense, marks
        self.d = tagset_dict(ts)
        self.ot = oracle_tables(ts)
        self._want, self._reads, self._batches = {}, {}, {}

    def reads(self, orientation):
        if orientation not in self._reads:
            self._reads[orientation] = strands(self.sense, orientation)
        return self._reads[orientation]

    def want(self, orientation, allow_ns=False):
        key = (orientation, bool(allow_ns))
        if key not in self._want:
            rs = self.reads(orientation)
            buf = np.frombuffer("".join(rs).encode("latin-1") + b"\0", dtype=np.uint8)
            off = np.zeros(len(rs) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(r) for r in rs], dtype=np.uint64)
            res, cnt = self.ot.decombine_batch_mt(buf, off, nat.ORIENTATIONS[orientation], allow_ns, 130, n_threads=8)
            rec = pu.oracle_to_records(res)
            rec.flags.writeable = False
            cnt.flags.writeable = False
            self._want[key] = (rec, cnt)
        return self._want[key]

    def batches(self, orientation):
        """[(read indices, packed batch)]: one batch per register shape of the kernels (reads of up to 160, 320 and
        511 nt), so that a few long reads do not move the short ones to another shape."""
        if orientation not in self._batches:
            rs = self.reads(orientation)
            cls = np.searchsorted([160, 320], [len(r) for r in rs], side="left")
            self._batches[orientation] = [(idx, nat.pack_reads([rs[i] for i in idx]))
                                          for idx in (np.nonzero(cls == c)[0] for c in range(3)) if len(idx)]
        return self._batches[orientation]

    def check(self, backend, orientation, allow_ns=False, flags=0, what=""):
        """The batches through a parity_util.Backend: every record and every counter against the oracle."""
        rs = self.reads(orientation)
        orec, ocnt = self.want(orientation, allow_ns)
        rec = np.zeros(len(rs), dtype=nat.RECORD_DTYPE)
        cnt = np.zeros(nat.N_COUNTERS, dtype=np.uint64)
        for idx, batch in self.batches(orientation):
            r, c = backend.run(batch, orientation, allow_ns, 130, flags)
            rec[idx] = r
            cnt += c
        pu.assert_records_equal(rec, orec, rs, f"{what} {orientation}")
        pu.assert_counters_equal(cnt, ocnt, f"{what} {orientation}")
        return rec, cnt

    @functools.cached_property
    def report(self) -> dict:
        """The figures behind the conditions on a contested workload: the oracle on the sense strand, the marks."""
        orec, ocnt = self.want("forward")
        return family.contest_report(self.ts, self.sense, self.marks, orec, ocnt, list(orc.COUNTER_NAMES))


@functools.lru_cache(maxsize=None)
def contested(split: str, n: int, p_v: float = 0.5) -> Workload:
    ts = tagset(split)
    sense, marks = family.contested_reads(ts, np.random.default_rng(SEEDS[split] + n % 997), n, p_v=p_v)
    return Workload(ts, sense, marks)


@functools.lru_cache(maxsize=None)
def ladder(split: str, n: int) -> Workload:
    ts = tagset(split)
    sense, marks = family.decoy_ladder(ts, np.random.default_rng(2 * SEEDS[split] + n % 997), n)
    return Workload(ts, sense, marks)


@functools.lru_cache(maxsize=None)
def ladder_report(w: Workload) -> dict:
    """From the oracle's side: per k, the reads whose ladder of k rungs the oracle's findall sees (k or more hits of
    one kind of half on that side), and the split of the statuses between decombined and found...not... exits."""
    orec, _ = w.want("forward")
    hits = np.array([family.half_hits(w.ot, r) for r in w.sense])
    seen_v, seen_j = hits[:, :2].max(axis=1), hits[:, 2:].max(axis=1)
    rep = {"reads": len(w.sense), "decombined": int((orec["status"] == 0).sum()),
           "found_not": int(np.isin(orec["status"], FOUND_NOT).sum())}
    for k in family.LADDER_KS:
        rep[f"v{k}"] = int(((w.marks["k_v"] == k) & (seen_v >= k)).sum())
        rep[f"j{k}"] = int(((w.marks["k_j"] == k) & (seen_j >= k)).sum())
    return rep


def assert_ladder_conditions(rep: dict, per_k: int):
    for k in family.LADDER_KS:
        assert rep[f"v{k}"] >= per_k and rep[f"j{k}"] >= per_k, rep
    assert rep["decombined"] >= 0.10 * rep["reads"] and rep["found_not"] >= 0.10 * rep["reads"], rep
