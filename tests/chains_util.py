"""Helpers of the multi-chain tests (test_chains.py on CPU, test_gpu_chains.py on the GPU): the TINY fixtures of both
chains in one work directory, synthetic two-chain FASTQ pairs, and the comparison of a `-c a,b` run's files with those of
the single-chain runs."""
import gzip
import json
import os

import numpy as np

from decombinator_amd import _native as nat
from decombinator_amd import pipeline, synth
from oracle import oracle as orc
from tests import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))
TIME_LINES = ("Directory,", "DateFinished,", "TimeFinished,", "TimeTaken")


def tiny_fixtures():
    return {c: json.load(open(os.path.join(HERE, "golden", f"tiny_{c}.json"))) for c in ("alpha", "beta")}


def _tagset(ts: dict) -> synth.TagSet:
    return synth.TagSet(species=ts["species"], tags=ts["tags"], chain=ts["chain"], v_tags=ts["v_tags"], v_jumps=ts["v_jumps"],
                        v_names=ts["v_names"], v_regions=ts["v_regions"], j_tags=ts["j_tags"], j_jumps=ts["j_jumps"],
                        j_names=ts["j_names"], j_regions=ts["j_regions"])


def tiny_workdir(workdir):
    """Both TINY tag sets in one tag directory and the (shared) TINY_1/2.fq pair in `workdir`."""
    fx = tiny_fixtures()
    assert fx["alpha"]["fastq_r1"] == fx["beta"]["fastq_r1"] and fx["alpha"]["fastq_r2"] == fx["beta"]["fastq_r2"]
    for f in fx.values():
        _tagset(f["tagset"]).write(str(workdir / "tags"))
    (workdir / "TINY_1.fq").write_text(fx["alpha"]["fastq_r1"])
    (workdir / "TINY_2.fq").write_text(fx["alpha"]["fastq_r2"])
    return fx


class OracleTables(nat.Tables):
    """nat.Tables that also carries the oracle's tables for the same tag set (the CPU tests' device stand-in)."""

    def __init__(self, v_tags, v_jumps, v_regions, j_tags, j_jumps, j_regions, v_half_split, j_half_split):
        super().__init__(v_tags, v_jumps, v_regions, j_tags, j_jumps, j_regions, v_half_split, j_half_split)
        self.oracle = orc.OracleTables(list(v_tags), list(v_jumps), [r.upper() for r in v_regions], list(j_tags),
                                       list(j_jumps), [r.upper() for r in j_regions], v_half_split, j_half_split)


class OracleDevice:
    """Stands the oracle in for nat.decombine and nat.decombine_chains, and counts the calls."""

    def __init__(self, monkeypatch):
        self.single_calls = 0
        self.chains_calls = []          # reads per decombine_chains call
        monkeypatch.setattr(nat, "Tables", OracleTables)
        monkeypatch.setattr(nat, "decombine", self.decombine)
        monkeypatch.setattr(nat, "decombine_chains", self.decombine_chains)

    @staticmethod
    def _one(tables, reads, orientation, allow_ns, lenthreshold):
        rec, cnt = pu.oracle_records(tables.oracle, reads, orientation, allow_ns, lenthreshold)
        return rec, cnt.astype(np.uint64)

    def decombine(self, tables, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0):
        self.single_calls += 1
        return self._one(tables, nat.unpack_reads(batch), orientation, allow_ns, lenthreshold)

    def decombine_chains(self, tables_list, batch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0):
        self.chains_calls.append(batch.n_reads)
        reads = nat.unpack_reads(batch)
        return [self._one(t, reads, orientation, allow_ns, lenthreshold) for t in tables_list]


def log_lines(path):
    return [ln for ln in open(path).read().split("\n") if not ln.startswith(TIME_LINES)]


def out_files(d):
    """{relative path: bytes (decompressed for .gz)} of what a run wrote under `d` (summary logs: without time lines)."""
    got = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            rel = os.path.relpath(p, d)
            if rel.startswith("Logs"):
                got[rel] = "\n".join(log_lines(p)).encode()
            elif f.endswith(".gz"):
                got[rel[:-3]] = gzip.open(p).read()
            else:
                got[rel] = open(p, "rb").read()
    return got


def write_synth_pair(workdir, tagsets, n_per_chain, seed, sub_rate=0.005, n_long=0, r1_mode=False, name="SYN"):
    """A FASTQ pair (or, with r1_mode, one file of barcode-read / second-read record pairs) of reads drawn half from each
    chain's germlines (interleaved), `n_long` of them stretched beyond 511 nt, with M13-style barcodes."""
    rng = np.random.default_rng(seed)
    per = []
    for k, ts in enumerate(tagsets):
        t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
        b = nat.synth_reads_host(t, nat.synth_cfg(seed=seed + k, sub_rate=sub_rate, n_rate=0.002), 0, n_per_chain)
        per.append(nat.unpack_reads(b))
    reads = [r for pair in zip(*per) for r in pair]
    for i in rng.choice(len(reads), size=n_long, replace=False):
        reads[i] = "".join(rng.choice(list("ACGT"), size=300)) + reads[i] + "".join(rng.choice(list("ACGT"), size=200))
    bcs = ["GTCGTGACTGGGAAAACCCTGG" + "".join(rng.choice(list("ACGTN"), size=6, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
           + "GTCGTGAT" + "".join(rng.choice(list("ACGT"), size=6)) for _ in range(len(reads))]
    if r1_mode:
        with open(workdir / f"{name}_1.fq", "w") as f1:
            for i, r in enumerate(reads):
                f1.write(f"@{name}:{i}:1 1:N\n{bcs[i]}{r}\n+\n{'I' * (len(bcs[i]) + len(r))}\n")
                f1.write(f"@{name}:{i}:2 2:N\n{r[:80]}\n+\n{'I' * len(r[:80])}\n")
    else:
        with open(workdir / f"{name}_1.fq", "w") as f1, open(workdir / f"{name}_2.fq", "w") as f2:
            for i, r in enumerate(reads):
                f1.write(f"@{name}:{i}:1 1:N\n{r}\n+\n{'I' * len(r)}\n")
                f2.write(f"@{name}:{i}:1 2:N\n{bcs[i]}{r[:40]}\n+\n{'I' * (len(bcs[i]) + 40)}\n")
    return len(reads)


def compare_with_single_runs(workdir, chains: str, argv_tail: list, command="decombine"):
    """Runs `<command> -c <chains>` in workdir/multi and `-c <item>` for each item in workdir/single_<item>, and asserts
    that every file the list run wrote equals the single runs' files, byte for byte (logs without their time lines).
    Returns the files of the list run."""
    from decombinator_amd import decombine as dec
    items = chains.split(",")
    (workdir / "multi").mkdir()
    pipeline.main([command, "-c", chains, "-op", "multi/"] + argv_tail)
    multi_counts = {c: dict(v) for c, v in dec.chain_counts.items()}
    got = out_files(workdir / "multi")
    want = {}
    for item in items:
        d = workdir / f"single_{item}"
        d.mkdir()
        pipeline.main([command, "-c", item, "-op", f"single_{item}/"] + argv_tail)
        letter = dec.resolve_chain_list([item])[0]
        single = {k: v for k, v in dec.counts.items() if k not in ("start_time", "end_time")}
        assert {k: v for k, v in multi_counts[letter].items() if k not in ("start_time", "end_time")} == single, item
        want.update(out_files(d))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    return got
