"""Helpers of the barcode-free count tests (test_nbc_count.py on CPU, test_gpu_nbc_count.py on the GPU): the expectation
(the oracle's per-read DCRs fed to a collections.Counter), clonal synthetic FASTQ with exception bytes inside inserts, and an
oracle-backed stand-in for nat.count_dcrs / nat.DcrCounts for the CPU tests."""
import collections
import os

import numpy as np

from decombinator_amd import _native as nat
from decombinator_amd import decombine as dec
from decombinator_amd import synth
from tests import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))


def read_dcrs(oracle_tables, reads, orientation="reverse", allow_ns=False, lenthreshold=130):
    """Per read: its DCR as the `.n12` row's first five fields joined by ", ", or None (the oracle's dcr())."""
    rec, cnt = pu.oracle_records(oracle_tables, reads, orientation, allow_ns, lenthreshold)
    out = []
    for k, r in enumerate(rec):
        if int(r["status"]) != 0:
            out.append(None)
            continue
        frame_read = reads[k] if int(r["frame"]) == 1 else dec.revcomp(reads[k])
        s, l = int(r["ins_start"]), int(r["ins_len"])
        out.append(", ".join([str(int(r["v"])), str(int(r["j"])), str(int(r["vdel"])), str(int(r["jdel"])), frame_read[s:s + l]]))
    return out, cnt


def expected_nbc(keys) -> str:
    """The `.nbc` text of per-read DCR keys in file order: Counter(...).most_common(), one "key, count" line each."""
    return "".join(f"{k}, {n}\n" for k, n in collections.Counter(k for k in keys if k is not None).most_common())


def counted_text(counted: dict) -> str:
    return nat.format_counts(counted).decode("latin-1")


class OracleCounts:
    """Stands in for nat.DcrCounts: a Counter of DCR keys with each key's first ordinal, read back as dcrx_counts_read's
    arrays (most_common() order)."""

    def __init__(self):
        self.counter = collections.Counter()
        self.first = {}

    def add(self, key: tuple, ordinal: int):
        self.counter[key] += 1
        self.first[key] = min(self.first.get(key, ordinal), ordinal)

    def read(self) -> dict:
        items = sorted(self.counter.items(), key=lambda kv: (-kv[1], self.first[kv[0]]))
        ins = [k[4].encode("latin-1") for k, _ in items]
        off = np.zeros(len(items) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in ins], dtype=np.uint64)
        return {"v": np.array([k[0] for k, _ in items], np.uint16), "j": np.array([k[1] for k, _ in items], np.uint16),
                "vdel": np.array([k[2] for k, _ in items], np.uint8), "jdel": np.array([k[3] for k, _ in items], np.uint8),
                "count": np.array([n for _, n in items], np.uint64), "first": np.array([self.first[k] for k, _ in items], np.uint64),
                "ins_off": off, "ins_text": b"".join(ins)}

    def reset(self):
        self.counter.clear()
        self.first.clear()

    def close(self):
        pass


class OracleCountDevice:
    """Stands the oracle in for nat.count_dcrs (and nat.DcrCounts); records the reads and ordinals of every call."""

    def __init__(self, monkeypatch):
        from tests import chains_util as chu
        self.calls = []             # (n_reads, n_chains, first_index, index given)
        monkeypatch.setattr(nat, "Tables", chu.OracleTables)
        monkeypatch.setattr(nat, "DcrCounts", OracleCounts)
        monkeypatch.setattr(nat, "count_dcrs", self.count_dcrs)

    def count_dcrs(self, tables_list, batch, counts_list, first_index=0, index=None, orientation="reverse", allow_ns=False,
                   lenthreshold=130):
        reads = nat.unpack_reads(batch)
        self.calls.append((len(reads), len(tables_list), int(first_index), index is not None))
        out = []
        for t, dc in zip(tables_list, counts_list):
            rec, cnt = pu.oracle_records(t.oracle, reads, orientation, allow_ns, lenthreshold)
            for k in np.nonzero(rec["status"] == 0)[0]:
                r = rec[k]
                frame_read = reads[k] if int(r["frame"]) == 1 else dec.revcomp(reads[k])
                s, l = int(r["ins_start"]), int(r["ins_len"])
                key = (int(r["v"]), int(r["j"]), int(r["vdel"]), int(r["jdel"]), frame_read[s:s + l])
                dc.add(key, int(first_index) + (int(index[k]) if index is not None else int(k)))
            out.append(cnt.astype(np.uint64))
        return out


def oracle_for(ts):
    from oracle import oracle as orc
    vs, js = ts.half_splits
    return orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                            [r.upper() for r in ts.j_regions], vs, js)


_IUPAC = "RYKMSWBDHVN"


def clonal_reads(ts, n_reads, seed, n_pool=300, zipf=1.2, orientation="reverse", exceptions=0.0, lower=0.0, n_long=0,
                 with_n=False):
    """n_reads reads drawn from a pool of synthetic reads of `ts` with Zipf weights (the top clone holds a large share).
    `exceptions` / `lower`: the share of pool reads whose insert gets an IUPAC byte (N among them only when with_n) / a lower
    case base; `n_long` pool reads stretched past 511 nt.  Returns the reads in file order."""
    rng = np.random.default_rng(seed)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    b = nat.synth_reads_host(t, nat.synth_cfg(seed=seed, p_rearranged=0.85, sub_rate=0.003, n_rate=0.0), 0, n_pool)
    pool = nat.unpack_reads(b)
    if orientation in ("forward", "both"):
        flip = rng.random(n_pool) < (1.0 if orientation == "forward" else 0.5)
        pool = [dec.revcomp(r) if f else r for r, f in zip(pool, flip)]
    rec, _ = pu.oracle_records(oracle_for(ts), pool, orientation, True, 130)
    iupac = _IUPAC if with_n else _IUPAC.replace("N", "")
    for k in range(n_pool):
        r = rec[k]
        if int(r["status"]) != 0 or int(r["ins_len"]) == 0:
            continue
        read = list(pool[k])
        L = len(read)
        for share, make in ((exceptions, lambda c: iupac[rng.integers(len(iupac))]), (lower, lambda c: c.lower())):
            if rng.random() < share:
                s = int(r["ins_start"]) + int(rng.integers(int(r["ins_len"])))
                q = s if int(r["frame"]) == 1 else L - 1 - s
                read[q] = make(read[q])
        pool[k] = "".join(read)
    for k in rng.choice(n_pool, size=n_long, replace=False):
        pool[k] = "".join(rng.choice(list("ACGT"), size=320)) + pool[k] + "".join(rng.choice(list("ACGT"), size=260))
    w = 1.0 / np.arange(1, n_pool + 1) ** zipf
    return [pool[i] for i in rng.choice(n_pool, size=n_reads, p=w / w.sum())]


def write_fastq(path, reads, fasta=False):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(f">r{i}\n{r}\n" if fasta else f"@r{i} 1:N\n{r}\n+\n{'I' * len(r)}\n")


def workdir_with(tmp_path, ts, reads, name="NBC_1.fq", fasta=False):
    ts.write(str(tmp_path / "tags"))
    write_fastq(tmp_path / name, reads, fasta)
    return ["-in", name, "-br", "R2", "-nbc", "--count-dcrs", "-tfdir", "tags", "-tg", ts.tags, "-sp", ts.species, "-c", ts.chain,
            "-dc"]
