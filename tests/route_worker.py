"""Worker of tests/test_gpu_parity.py::test_first_call_both_with_one_frame_fused_and_one_not: a process of its own, because the
library reads DCRX_DEBUG_FUSE_LIMIT_KB once per process.  Under a limit of 54 KB config 2's reverse frame (53 152 bytes)
fuses and its forward frame (56 608 bytes) does not.  5 000 device-resident reads through dcrx_decombine_device:
  handle A   both, both             the very first call needs the tail list for its second pass
  handle B   reverse, reverse with DCRX_F_V2_NO_FUSE      a handle that has fused so far, then a call that does not
Every record and counter of every call against the oracle, and the launch forms the handle reports."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decombinator_amd import _native as nat          # noqa: E402
from decombinator_amd import synth                   # noqa: E402
from oracle import oracle as orc                     # noqa: E402
from tests import parity_util as pu                  # noqa: E402

N = 5000
FUSED, ROLE = "v2, tail inside the scan", "v2, tail as a role"


def main():
    ts = synth.config_tagset(2)
    vs, js = ts.half_splits
    ot = orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                          [r.upper() for r in ts.j_regions], vs, js)
    cfg = nat.synth_cfg(seed=63, sub_rate=0.01)
    want = {}

    def run(t, db, reads, orientation, flags, what):
        d_rec = nat.DeviceBuffer(N * 16)
        d_cnt = nat.DeviceBuffer(nat.N_COUNTERS * 8)
        nat.check(nat.lib().dcrx_memset_device(d_rec.ptr, 0xEE, N * 16))      # (a record no kernel writes would show)
        nat.decombine_device(t, db, d_rec, d_cnt, orientation=orientation, flags=flags)
        nat.synchronize()
        if orientation not in want:
            want[orientation] = pu.oracle_records(ot, reads, orientation, False, 130)
        pu.assert_records_equal(d_rec.to_host(nat.RECORD_DTYPE, N), want[orientation][0], reads, what)
        pu.assert_counters_equal(d_cnt.to_host(np.uint64, nat.N_COUNTERS), want[orientation][1], what)
        return {o: t.tune_state(N, o)["launch_form"] for o in ("reverse", "forward")}

    # (the reads come from a handle of their own: the handles under test meet the device in their first decombine call)
    gen = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, vs, js)
    assert gen.info()["v2_scan_bytes"] == 56608, gen.info()      # the larger of the two frames' pair tables: the forward frame's
    db = nat.synth_reads_device(gen, cfg, 0, N)
    reads = nat.unpack_reads(nat.synth_reads_host(gen, cfg, 0, N))

    def handle():
        return nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, vs, js)

    t = handle()
    for k in (1, 2):
        forms = run(t, db, reads, "both", 0, f"both, call {k} of a fresh handle")
        assert forms == {"reverse": FUSED, "forward": ROLE}, (k, forms)
    t = handle()
    forms = run(t, db, reads, "reverse", 0, "reverse")
    assert forms == {"reverse": FUSED, "forward": "none yet"}, forms
    forms = run(t, db, reads, "reverse", nat.F_V2_NO_FUSE, "reverse, tail as a role")
    assert forms == {"reverse": ROLE, "forward": "none yet"}, forms
    print("ROUTE_OK")


if __name__ == "__main__":
    main()
