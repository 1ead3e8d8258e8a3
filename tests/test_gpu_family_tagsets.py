"""The v2 kernels on gene-family tag sets (oracle/family.py): tags one and two substitutions apart that share a half,
related regions, decoy half tags.  A window of a read is then within Hamming 1 of several tags, a half-tag keyword maps
to three to six tags, and the reference's candidate order (half-tag hits in findall order, genes in index order, the
first that passes Hamming <= 1 and whose walk succeeds) decides the record — on every launch form, every record and
every counter against the oracle.  The conditions that keep these tests from passing on nothing are asserted on the
oracle's results and the generator's marks (tests/test_family_tagsets.py asserts them on the CPU as well)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat
from oracle import casegen, family
from tests import family_util as fu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ["original", "extended"]
N_CONTESTED, N_LADDER = 60_000, 40_000


def _backend(split):
    be = pu.Backend("hip", fu.tagset_dict(fu.tagset(split)))
    info = be.tables.info()
    assert info["equal_len_per_automaton"] and info["v2_tables"], info
    return be


def _form(be, n, orientation):
    return be.tables.tune_state(n, orientation)["launch_form"]


def test_family_fixture_runs_on_the_v2_kernels():
    """tests/golden/dcr_family_original_b.json.gz (from the reference itself) takes the v2 kernels, so the flag variants of
    tests/test_gpu_parity.py::test_hip_matches_golden_and_oracle are that many different paths on it."""
    from tests import golden_util as gu
    fx = gu.load(os.path.join(gu.GOLDEN_DIR, "dcr_family_original_b.json.gz"))
    t = pu.native_tables(fx["tagset"])
    assert t.info()["v2_tables"] and t.info()["equal_len_per_automaton"]
    reads = [c["read"] for c in fx["cases"] if c["orientation"] == "reverse" and not c["allowNs"] and c["lenthreshold"] == 130]
    assert len(reads) > 500
    nat.decombine(t, nat.pack_reads(reads), flags=0)
    form = t.tune_state(len(reads))["launch_form"]
    print("launch form:", form)
    assert form.startswith("v2"), form


@pytest.mark.parametrize("flags", [0, nat.F_V2_NO_FUSE, nat.F_V2_NO_LEAN_RESCUE, nat.F_V2_LEAN_SERIAL, nat.F_V2_SHAPE(3), nat.F_V1_KERNELS],
                         ids=["v2", "v2-tail-as-a-role", "v2-general-form-only", "v2-separate-launches", "v2-one-read-per-lane", "v1-pairscan"])
@pytest.mark.parametrize("orientation,allow_ns", [("reverse", False), ("forward", False), ("both", False), ("both", True)],
                         ids=["reverse", "forward", "both", "both-allowNs"])
@pytest.mark.parametrize("split", SPLITS)
def test_contested_reads_on_every_launch_form(split, orientation, allow_ns, flags):
    w = fu.contested(split, N_CONTESTED)
    print(w.report)
    family.assert_contest_conditions(w.report)
    be = _backend(split)
    w.check(be, orientation, allow_ns=allow_ns, flags=flags, what=f"contested, flags {flags}")
    form = _form(be, N_CONTESTED, orientation)
    print("launch form:", form)
    assert form == "three-launch form" if flags == nat.F_V1_KERNELS else form.startswith("v2"), form


def _device_generator_batches(t, kind, sub_rate, seed):
    """(reads in their stored strand, stride) of one kind of batch."""
    import random
    if kind == "uniform-150":
        return nat.unpack_reads(nat.synth_reads_host(t, nat.synth_cfg(seed=seed, sub_rate=sub_rate, n_rate=0.002), 0, 300_000)), None
    if kind == "ragged":          # cut as tests/test_gpu_parity.py::test_ragged_lengths_and_empty_reads cuts
        rng = np.random.default_rng(11)
        reads = nat.unpack_reads(nat.synth_reads_host(t, nat.synth_cfg(seed=seed, read_len=320, sub_rate=sub_rate, n_rate=0.002), 0, 300_000, stride=80))
        cut = rng.integers(0, 321, size=len(reads))
        start = rng.integers(0, 120, size=len(reads))
        reads = [r[s:s + c] if i % 3 else r[:c] for i, (r, s, c) in enumerate(zip(reads, start, cut))]
        reads[0] = reads[-1] = ""
        return reads, 80
    if kind == "300-nt":
        return nat.unpack_reads(nat.synth_reads_host(t, nat.synth_cfg(seed=seed, read_len=300, sub_rate=sub_rate, n_rate=0.002), 0, 300_000,
                                                     stride=nat.stride_for(300))), nat.stride_for(300)
    rng = random.Random(7)        # the long form: 6 000 reads lengthened to 600 nt
    cores = nat.unpack_reads(nat.synth_reads_host(t, nat.synth_cfg(seed=seed, p_rearranged=0.8, sub_rate=sub_rate, n_rate=0.002), 0, 6000))
    out = []
    for r in cores:
        a = rng.randrange(0, 600 - len(r) + 1)
        flank = "".join(rng.choices("ACGT", k=600 - len(r)))
        out.append(flank[:a] + r + flank[a:])
    return out, None


@pytest.mark.parametrize("kind", ["uniform-150", "ragged", "300-nt", "600-nt-long-form"])
@pytest.mark.parametrize("sub_rate", [0.005, 0.02, 0.05])
def test_family_reads_from_the_device_generator(sub_rate, kind):
    """The generator's reads (they start 20-60 nt upstream of the V tag, so the regions' decoy half tags lie inside part of
    them) on a family set with decoys and related regions: `reverse` on the generator's strand, `both` with every other read
    turned to the sense strand."""
    w = fu.Workload(fu.tagset("original"), [], np.zeros(0, dtype=family.MARKS_DTYPE))
    be = _backend("original")
    stored, stride = _device_generator_batches(be.tables, kind, sub_rate, seed=int(sub_rate * 1000))
    n_ok = 0
    for orientation in ("reverse", "both"):
        reads = stored if orientation == "reverse" else [casegen.revcomp(r) if i % 2 else r for i, r in enumerate(stored)]
        batch = nat.pack_reads(reads, stride=stride)
        rec, cnt = be.run(batch, orientation)
        buf = np.frombuffer("".join(reads).encode("latin-1") + b"\0", dtype=np.uint8)
        off = np.zeros(len(reads) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
        ores, ocnt = w.ot.decombine_batch_mt(buf, off, nat.ORIENTATIONS[orientation], False, 130, n_threads=8)
        pu.assert_records_equal(rec, pu.oracle_to_records(ores), reads, f"{kind} {sub_rate} {orientation}")
        pu.assert_counters_equal(cnt, ocnt, f"{kind} {sub_rate} {orientation}")
        n_ok += int((ores["status"] == 0).sum())
        if kind != "600-nt-long-form":
            assert _form(be, len(reads), orientation).startswith("v2")
        print(kind, sub_rate, orientation, "decombined", int((ores["status"] == 0).sum()), "of", len(reads),
              {k: int(ocnt[nat.COUNTER_NAMES.index(k)]) for k in ("verr1", "verr2", "jerr1", "jerr2", "frame_forward")},
              "form:", _form(be, len(reads), orientation))
    assert n_ok > len(stored) // 10


@pytest.mark.parametrize("orientation", ["reverse", "forward", "both"])
@pytest.mark.parametrize("split", SPLITS)
def test_decoy_ladder_at_the_list_limits(split, orientation):
    """k = 3 .. 10 bare half tags beside the tag's own hit: on both sides of the lean rescue's four flagged pairs per side,
    of the eight events of an entry and of the eight hits of a hit list; the reads in one batch per register shape (up to
    160, 320 and 511 nt)."""
    w = fu.ladder(split, N_LADDER)
    rep = fu.ladder_report(w)
    print(rep, "reads per shape:", [len(idx) for idx, _ in w.batches(orientation)])
    fu.assert_ladder_conditions(rep, per_k=2000)
    assert len(w.batches(orientation)) == 3
    be = _backend(split)
    w.check(be, orientation, what="ladder")
    form = _form(be, N_LADDER, orientation)
    print("launch form:", form)
    assert form.startswith("v2"), form


def _child(args, env, timeout):
    return subprocess.run([sys.executable] + args, env=dict(os.environ, DCRX_DEBUG_FLAGS="1", PYTHONPATH=ROOT, **env), cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_contested_reads_with_list_e_inside_the_scan():
    """The forced form with list E's entries finished inside the scan kernel (DCRX_DEBUG_FUSE_E, read once per process: a
    child): it takes batches of one length, so 60 000 contested reads of 150 nt — the smallest batch tried at which the
    worker's tune_state says so — every record and counter against the threaded oracle, two calls."""
    p = _child([os.path.join(ROOT, "tests", "forced_shape_worker.py"), "family", str(N_CONTESTED), "2"], {"DCRX_DEBUG_FUSE_E": "1"}, 300)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and "SHAPE_OK" in p.stdout and "tail and list E inside the scan" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])


RING_WORKER = r'''
import numpy as np
from decombinator_amd import _native as nat
from oracle import family
from tests import family_util as fu, parity_util as pu
ts = fu.tagset("original")
sense, marks = family.contested_reads(ts, np.random.default_rng(5), 50_000, p_v=1 / 3, p_j=0.0, p_sub=0.0, p_cut=0.0,
                                      lengths=(150,), length_p=(1.0,))
order = np.random.default_rng(6).permutation(200_000) % 50_000
w = fu.Workload(ts, [sense[i] for i in order], marks[order])
rep = w.report
print(rep)
assert rep["marked_v_decombined"] > 40_000 and rep["contested_v"] >= 0.95 * rep["marked_v_decombined"], rep
assert rep["decombined"] > 150_000, rep          # every read a rearrangement: the tail ring runs full beside the event entries
be = pu.Backend("hip", w.d)
for orientation in ("reverse", "forward"):
    w.check(be, orientation, what="ring")
    print("form", be.tables.tune_state(200_000, orientation)["launch_form"])
print("ok")
'''


@pytest.mark.parametrize("ring", ["4", "16"])
def test_fused_ring_with_contested_tail_reads(ring):
    """The tail inside the scan kernel with the shortest ring and the longest (DCRX_DEBUG_RING_BATCHES, read once per
    process: a child), as tests/test_gpu_parity.py::test_fused_tail_ring_under_pressure runs it: 200 000 reads, every one a
    rearrangement (two thirds are tail reads that fill the ring as fast as the scanning waves can), a third contested (event
    entries between them)."""
    p = _child(["-c", RING_WORKER], {"DCRX_DEBUG_RING_BATCHES": ring}, 300)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and "ok" in p.stdout and "v2, tail inside the scan" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])


def test_two_family_chains_in_one_pass():
    """An alpha-like and a beta-like family set through dcrx_decombine_chains_count over 200 000 mixed reads: per chain the
    counted table equals the single entry's and the Counter built from dcrx_decombine's records (in the DCR count
    neighbouring genes differ in the `v` or `j` field of the key alone), and the records are the oracle's."""
    from tests.test_gpu_nbc_count import _expected, _got
    wa, wb = fu.contested("extended", N_CONTESTED), fu.contested("original", N_CONTESTED)
    reads = wa.reads("reverse") + wb.reads("reverse") + wa.reads("reverse")[:40_000] + wb.reads("reverse")[:40_000]
    assert len(reads) == 200_000
    np.random.default_rng(1).shuffle(reads)
    batch = nat.pack_reads(reads)
    tables = [pu.native_tables(wa.d), pu.native_tables(wb.d)]
    dcs = [nat.DcrCounts(), nat.DcrCounts()]
    cnts = nat.decombine_chains_count(tables, batch, dcs, 5)
    for w, t, dc, cnt in zip((wa, wb), tables, dcs, cnts):
        single = nat.DcrCounts()
        c1 = nat.decombine_count(t, batch, single, 5)
        assert (c1 == cnt).all()
        got = _got(dc.read())
        assert got == _got(single.read()) and len(got) > 10_000
        rec, cnt2 = nat.decombine(t, batch)
        assert (cnt2 == cnt).all()
        assert got == _expected(rec, batch, 5)
        orec, ocnt = pu.oracle_records(w.ot, reads, "reverse", False, 130)
        pu.assert_records_equal(rec, orec, reads, w.ts.chain)
        pu.assert_counters_equal(cnt, ocnt, w.ts.chain)
        single.close()
        dc.close()
