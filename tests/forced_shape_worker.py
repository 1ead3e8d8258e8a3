"""Worker of tests/test_gpu_parity.py::test_timed_launch_shapes_at_size: one process per launch shape, because the library
reads its A/B switches (DCRX_DEBUG_RESCUE_WAVES, DCRX_DEBUG_TAIL_WAVES, DCRX_DEBUG_NO_TUNE) once per process.  Decombines
N device-resident reads of a BASELINE config in one launch (the fused form at a batch size the handle tunes itself on:
>= 2^20 reads), CALLS times on one handle — the handle's own choice of rescue waves settles on the sixth call — and compares
every record and every counter of every call with the threaded oracle.  usage: forced_shape_worker.py CONFIG N CALLS
CONFIG `family`: N uniform 150-nt contested reads of a gene-family tag set (oracle/family.py) instead of the generator's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decombinator_amd import _native as nat          # noqa: E402
from decombinator_amd import synth                   # noqa: E402
from oracle import oracle as orc                     # noqa: E402
from tests import parity_util as pu                  # noqa: E402


def family_main(n, calls):
    """Contested reads (windows within Hamming 1 of two tags) in one uniform batch, as the forms that need one length for
    all reads take them; the conditions on the workload from the oracle's side, then every record and counter."""
    from oracle import family
    from tests import family_util as fu
    ts = fu.tagset("original")
    sense, marks = family.contested_reads(ts, np.random.default_rng(n), n, p_cut=0.0, lengths=(150,), length_p=(1.0,))
    w = fu.Workload(ts, sense, marks)
    family.assert_contest_conditions(w.report, scale=n / 60_000)
    t = pu.native_tables(w.d)
    (_, hb), = w.batches("reverse")
    assert hb.lens is None and hb.read_len == 150
    orec, ocnt = w.want("reverse")
    db = nat.DeviceBatch.from_host(hb)
    d_rec = nat.DeviceBuffer(n * 16)
    d_cnt = nat.DeviceBuffer(nat.N_COUNTERS * 8)
    for k in range(calls):
        nat.check(nat.lib().dcrx_memset_device(d_rec.ptr, 0xEE, n * 16))
        nat.decombine_device(t, db, d_rec, d_cnt)
        nat.synchronize()
        pu.assert_records_equal(d_rec.to_host(nat.RECORD_DTYPE, n), orec, w.reads("reverse"), f"call {k}")
        pu.assert_counters_equal(d_cnt.to_host(np.uint64, nat.N_COUNTERS), ocnt, f"call {k}")
    print("SHAPE_OK", "family", n, calls, t.tune_state(n), w.report)


def main():
    if sys.argv[1] == "family":
        return family_main(int(sys.argv[2]), int(sys.argv[3]))
    config, n, calls = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    ts = synth.config_tagset(2) if config == 2 else list(synth.config5_tagsets())[0]
    vs, js = ts.half_splits
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, vs, js)
    ot = orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                          [r.upper() for r in ts.j_regions], vs, js)
    cfg = nat.synth_cfg(seed=config, sub_rate=0.02 if config == 5 else 0.005)
    hb = nat.synth_reads_host(t, cfg, 0, n)
    buf, offsets = nat.unpack_reads_raw(hb)
    ores, ocnt = ot.decombine_batch_mt(buf, offsets)
    orec = pu.oracle_to_records(ores)
    db = nat.synth_reads_device(t, cfg, 0, n)
    d_rec = nat.DeviceBuffer(n * 16)
    d_cnt = nat.DeviceBuffer(nat.N_COUNTERS * 8)
    for k in range(calls):
        nat.check(nat.lib().dcrx_memset_device(d_rec.ptr, 0xEE, n * 16))      # (a record no kernel writes would show)
        nat.decombine_device(t, db, d_rec, d_cnt)
        nat.synchronize()
        rec = d_rec.to_host(nat.RECORD_DTYPE, n)
        cnt = d_cnt.to_host(np.uint64, nat.N_COUNTERS)
        if rec.tobytes() != orec.tobytes():
            pu.assert_records_equal(rec, orec, nat.unpack_reads(hb), f"call {k}")
        pu.assert_counters_equal(cnt, ocnt, f"call {k}")
    st = t.tune_state(n)
    print("SHAPE_OK", config, n, calls, st)


if __name__ == "__main__":
    main()
