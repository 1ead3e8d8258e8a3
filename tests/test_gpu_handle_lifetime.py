"""What a tables handle (and a DcrCounts) owns on the device, over its life: one handle taken from a small batch to one large
enough to regrow every workspace and back — the device entry with the tuple sink off and on, the host entry, a count step —
with records, counters, messages and counts equal to the oracle's each time; then cycles of create, use and destroy, after
which the device's free memory must be where it was: a handle that is destroyed gives everything back."""
import collections
import subprocess
import sys

import numpy as np
import pytest

from decombinator_amd import _native as nat, synth
from tests import nbc_count_util as nu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

SMALL = 3_000            # below the smallest workspace (4 096 reads)
LARGE = 1_200_000        # regrows the lists, the sink, the staging and the count table; a size class the handle tunes itself on
ORDER = ("small", "large", "small")
CYCLES = 20

_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _tables(ts):
    return nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)


class _Case:
    """One batch on the host and on the device, and what the oracle says about it."""

    def __init__(self, t, ot, seed, n):
        self.n = n
        self.host = nat.synth_reads_host(t, nat.synth_cfg(seed=seed, n_rate=0.002), 0, n)
        self.dev = nat.DeviceBatch.from_host(self.host)
        self.raw, self.off = nat.unpack_reads_raw(self.host)
        res, self.cnt = ot.decombine_batch_mt(self.raw, self.off, nat.ORIENTATIONS["reverse"], False, 130, n_threads=8)
        self.rec = pu.oracle_to_records(res)

    def dcrs(self):
        """[(v, j, vdel, jdel, insert bytes, read)] of the reads the oracle decombined, in read order."""
        rec, raw = self.rec, self.raw.tobytes()
        ok = np.nonzero(rec["status"] == 0)[0]
        v, j, vd, jd, s, l, fr = (rec[f][ok].tolist() for f in ("v", "j", "vdel", "jdel", "ins_start", "ins_len", "frame"))
        o0, o1 = self.off[ok].tolist(), self.off[ok + 1].tolist()
        out = []
        for k, r in enumerate(ok.tolist()):
            if fr[k]:
                ins = raw[o0[k] + s[k]:o0[k] + s[k] + l[k]]
            else:
                e = o1[k] - s[k]
                ins = raw[e - l[k]:e][::-1].translate(_COMP)
            out.append((v[k], j[k], vd[k], jd[k], ins, r))
        return out


class _Fixture:
    def __init__(self):
        self.ts = synth.config_tagset(2)
        ot = nu.oracle_for(self.ts)
        t = _tables(self.ts)
        self.cases = {"small": _Case(t, ot, 71, SMALL), "large": _Case(t, ot, 72, LARGE)}
        self.codec_len = 150
        codec = nat.TupleCodec(t, self.codec_len)
        self.d_rec = nat.DeviceBuffer(LARGE * 16)
        self.d_cnt = nat.DeviceBuffer(nat.N_COUNTERS * 8)
        self.d_msg = nat.DeviceBuffer(codec.message_bytes(LARGE, LARGE) + 64)
        self.d_n = nat.DeviceBuffer(8)
        t.close()
        # the count of the three steps: one Counter, each key's first ordinal (step k's reads start at ordinal k * LARGE)
        c, first = collections.Counter(), {}
        for step, name in enumerate(ORDER):
            for key in self.cases[name].dcrs():
                c[key[:5]] += 1
                first.setdefault(key[:5], step * LARGE + key[5])
        self.want_counts = [k + (n, first[k]) for k, n in sorted(c.items(), key=lambda kv: (-kv[1], first[kv[0]]))]

    def free(self):
        for b in (self.d_rec, self.d_cnt, self.d_msg, self.d_n):
            b.free()


def _counted_rows(counted):
    text, off = counted["ins_text"], counted["ins_off"].tolist()
    cols = [counted[f].tolist() for f in ("v", "j", "vdel", "jdel", "count", "first")]
    return [(cols[0][k], cols[1][k], cols[2][k], cols[3][k], text[off[k]:off[k + 1]], cols[4][k], cols[5][k])
            for k in range(len(cols[0]))]


def _use(fx, t, dc, what):
    """Every entry over small, large, small on the one handle; everything that comes back against the oracle."""
    codec = nat.TupleCodec(t, fx.codec_len)
    for sink in (False, True):
        for name in ORDER:
            case, tag = fx.cases[name], f"{what}: device entry, sink {'on' if sink else 'off'}, {name}"
            n = case.n
            nat.check(nat.lib().dcrx_memset_device(fx.d_rec.ptr, 0xEE, n * 16))
            if sink:
                nat.check(nat.lib().dcrx_memset_device(fx.d_msg.ptr, 0xEE, codec.message_bytes(n, n)))
                nat.set_tuple_sink(t, codec, fx.d_msg.ptr, n, fx.d_n.ptr)
            try:
                nat.decombine_device(t, case.dev, fx.d_rec, fx.d_cnt)
                nat.synchronize()
            finally:
                if sink:
                    nat.set_tuple_sink(t, None)
            rec = fx.d_rec.to_host(nat.RECORD_DTYPE, n)
            pu.assert_records_equal(rec, case.rec, what=tag)
            pu.assert_counters_equal(fx.d_cnt.to_host(np.uint64, nat.N_COUNTERS), case.cnt, what=tag)
            if sink:
                k = int(fx.d_n.to_host(np.uint64, 1)[0])
                assert k == int((case.rec["status"] == 0).sum()), tag
                msg = fx.d_msg.to_host(np.uint8, codec.message_bytes(n, k))
                assert msg.tobytes() == codec.pack(case.rec, n_slots=n).tobytes(), f"{tag}: the message differs"
    for name in ORDER:
        case, tag = fx.cases[name], f"{what}: host entry, {name}"
        rec, cnt = nat.decombine(t, case.host)
        pu.assert_records_equal(rec, case.rec, what=tag)
        pu.assert_counters_equal(cnt, case.cnt, what=tag)
    for step, name in enumerate(ORDER):
        case = fx.cases[name]
        cnt = nat.decombine_count(t, case.host, dc, step * LARGE)
        pu.assert_counters_equal(cnt, case.cnt, what=f"{what}: count step, {name}")
    got = _counted_rows(dc.read())
    assert len(got) == len(fx.want_counts) and got == fx.want_counts, f"{what}: the counted DCRs differ from the oracle's"


def _free_bytes():
    """torch.cuda.mem_get_info() once the handle's work is over, read by a fresh interpreter: free memory is the device's,
    whichever process holds the rest, and the reader's own context costs every reading the same.  (Asked in this process,
    once libdcrx has initialised HIP, torch reports that no GPU is available.)"""
    nat.synchronize()
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.mem_get_info(0)[0])"],
                         capture_output=True, text=True, timeout=180, check=True)
    return int(out.stdout.split()[-1])


def test_a_handle_regrows_and_gives_everything_back():
    nat.check(nat.lib().dcrx_set_device(0))
    fx = _Fixture()
    try:
        t, dc = _tables(fx.ts), nat.DcrCounts()
        _use(fx, t, dc, "first handle")
        dc.close()
        t.close()
        free_after, footprint = [], None
        for cycle in range(1, CYCLES + 1):
            t, dc = _tables(fx.ts), nat.DcrCounts()
            _use(fx, t, dc, f"cycle {cycle}")
            dc.close()
            before = _free_bytes()
            t.close()
            free_after.append(_free_bytes())
            if cycle == 2:
                footprint = free_after[-1] - before       # what one live tables handle holds on the device
        drop = free_after[1] - free_after[-1]              # end of cycle 2 to end of the last cycle
        print(f"\nhandle lifetime: footprint F = {footprint} bytes; free memory after each cycle's destroy: {free_after}; "
              f"drop from cycle 2 to cycle {CYCLES} = {drop} bytes")
        assert footprint > 0, "a live handle holds device memory"
        assert drop < footprint, f"free device memory fell by {drop} bytes over {CYCLES - 2} cycles (a handle holds {footprint})"
    finally:
        fx.free()
