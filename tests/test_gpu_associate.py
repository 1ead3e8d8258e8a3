"""The permutation null on the device (include/dcrx.h "association"): both entries on every output cell against the contract
(tests/assoc_util.expected_permute) over the constructed cases — every sample count around a mask's seam, one case and one
control, the edges of a block's slice and of its relabelings (read from the host build), the three kinds of table, the tail of
0 and 1 ranks, the 64-bit tail cells, contention on one cell, multiplicities of 0, the extreme seeds —, outputs prefilled and
guarded, two calls on one stream without a wait between them, the refusals with every output byte left alone, what the device
entry makes of masks and tables it cannot check, and the stage end to end."""
import functools
import gzip
import os
from fractions import Fraction

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import associate as asc
from tests import assoc_util as au

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2
GUARD = 64
DTYPES = {"obs_rank": np.uint32, "labels": np.uint64, "perm_min": np.uint32, "tail": np.uint64}


@functools.lru_cache(maxsize=None)
def _want(name):
    args = au.constructed()[name]
    want = au.expected_permute(*args)
    au.premise(name, args, want)
    for key in au.OUTPUTS:
        want[key].setflags(write=False)
    return want


def _counts(args):
    return {"obs_rank": len(args[0]), "labels": args[7], "perm_min": args[7], "tail": args[6]}


class _Out:
    """An output array of exactly `count` entries with GUARD bytes behind it, 0xA5 all over before the call."""

    def __init__(self, dtype, count):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.bytes = self.count * self.dtype.itemsize
        self.buf = nat.DeviceBuffer.from_host(np.full(self.bytes + GUARD, 0xA5, np.uint8))
        self.ptr = self.buf.ptr

    def raw(self):
        return self.buf.to_host(np.uint8, self.bytes + GUARD)

    def read(self, written=None):
        raw = self.raw()
        assert (raw[self.bytes:] == 0xA5).all(), "written behind an output array"
        kept = self.bytes if written is None else int(written) * self.dtype.itemsize
        assert (raw[kept:self.bytes] == 0xA5).all(), "written behind what the call writes"
        return raw[:kept].view(self.dtype).copy()


def _outs(counts):
    return {k: _Out(DTYPES[k], counts[k]) for k in au.OUTPUTS}


def _inputs(args):
    masks, mults, N, C_, table = args[:5]
    return (nat.DeviceBuffer.from_host(np.ascontiguousarray(masks, np.uint64)), nat.DeviceBuffer.from_host(np.ascontiguousarray(mults, np.uint32)),
            nat.DeviceBuffer.from_host(np.ascontiguousarray(table, np.uint16)))


def _launch(args, inputs, outs, stream=None):
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = args
    nat.assoc_permute_device(N, C_, len(masks), inputs[0], inputs[1], inputs[2], n_ranks, tail_ranks, P, seed, outs["obs_rank"], outs["labels"],
                             outs["perm_min"], outs["tail"], stream)


@pytest.mark.parametrize("name", au.constructed_names())
def test_both_entries_against_the_contract(name):
    args = au.constructed()[name]
    want = _want(name)
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = args
    got = nat.assoc_permute(*args)
    au.assert_same(got, want, (name, "host entry"))
    assert got["stats"] == want["stats"], name
    n1 = bin(C_).count("1")
    assert all(bin(int(x)).count("1") == n1 and int(x) >> N == 0 for x in got["labels"])
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    au.assert_same({k: outs[k].read() for k in au.OUTPUTS}, want, (name, "device entry"))


def test_a_large_then_a_small_call_on_one_stream_without_a_wait():
    big, small = "past_both", "tail_1"
    a_big, a_small = au.constructed()[big], au.constructed()[small]
    assert all(0 < _counts(a_small)[k] < _counts(a_big)[k] for k in au.OUTPUTS)      # the small call fits the large one's arrays
    stream = nat.Stream()
    in_big, in_small = _inputs(a_big), _inputs(a_small)
    first, second = _outs(_counts(a_big)), _outs(_counts(a_small))
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, second, stream.ptr)
    stream.synchronize()
    au.assert_same({k: first[k].read() for k in au.OUTPUTS}, _want(big), "the large call")
    au.assert_same({k: second[k].read() for k in au.OUTPUTS}, _want(small), "the small call behind it")
    # and the small call into the large one's arrays, behind a second large call: its cells in front, the large call's behind
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, first, stream.ptr)
    stream.synchronize()
    for k in au.OUTPUTS:
        n, both = _counts(a_small)[k], first[k].read()
        assert np.array_equal(both[:n], np.asarray(_want(small)[k]).astype(DTYPES[k])), k
        assert np.array_equal(both[n:], np.asarray(_want(big)[k]).astype(DTYPES[k])[n:]), k


REFUSED = [({"N": 1, "C": 1}, E_INVALID), ({"N": 65}, E_INVALID), ({"C": 0}, E_INVALID), ({"C": 0xFFFF}, E_INVALID), ({"C": 1 << 16}, E_INVALID),
           ({"n_ranks": 0, "tail": 0}, E_INVALID), ({"n_ranks": 17 * 17 + 1}, E_INVALID), ({"tail": 82}, E_INVALID),
           ({"P": (1 << 20) + 1}, E_UNSUPPORTED), ({"F": 1 << 30}, E_UNSUPPORTED), ({"null": "mask"}, E_INVALID), ({"null": "tail"}, E_INVALID)]


@pytest.mark.parametrize("change,code", REFUSED)
def test_refusals_leave_every_output_byte_alone(change, code):
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = au.constructed()["F257"]
    a = dict({"N": N, "C": C_, "F": len(masks), "n_ranks": n_ranks, "tail": 5, "P": P}, **{k: v for k, v in change.items() if k != "null"})
    L = nat.lib()
    # the device entry, on device arrays
    inputs, outs = _inputs((masks, mults, N, C_, table)), _outs({"obs_rank": len(masks), "labels": P, "perm_min": P, "tail": 5})
    d_mask = None if change.get("null") == "mask" else inputs[0].ptr
    d_tail = None if change.get("null") == "tail" else outs["tail"].ptr
    rc = L.dcrx_assoc_permute_device(a["N"], a["C"], a["F"], d_mask, inputs[1].ptr, inputs[2].ptr, a["n_ranks"], a["tail"], a["P"], seed,
                                     outs["obs_rank"].ptr, outs["labels"].ptr, outs["perm_min"].ptr, d_tail, None)
    assert rc == code, L.dcrx_last_error()
    nat.synchronize()
    assert all((outs[k].raw() == 0xA5).all() for k in au.OUTPUTS)
    # the host entry, on host arrays
    host = {k: np.full(max(c, 1) * np.dtype(DTYPES[k]).itemsize, 0xA5, np.uint8) for k, c in (("obs_rank", len(masks)), ("labels", P), ("perm_min", P), ("tail", 5))}
    mk, ml, tb = np.ascontiguousarray(masks, np.uint64), np.ascontiguousarray(mults, np.uint32), np.ascontiguousarray(table, np.uint16)
    rc = L.dcrx_assoc_permute(a["N"], a["C"], a["F"], None if change.get("null") == "mask" else mk.ctypes.data, ml.ctypes.data, tb.ctypes.data,
                              a["n_ranks"], a["tail"], a["P"], seed, host["obs_rank"].ctypes.data, host["labels"].ctypes.data,
                              host["perm_min"].ctypes.data, None if change.get("null") == "tail" else host["tail"].ctypes.data, None)
    assert rc == code, L.dcrx_last_error()
    assert all((v == 0xA5).all() for v in host.values())


@pytest.mark.parametrize("what", ["mask", "cell", "weight"])
def test_what_the_host_entry_sees_in_the_arrays_is_refused_before_any_write(what):
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = au.constructed()["F257"]
    mk, ml, tb = np.array(masks, np.uint64), np.array(mults, np.uint32), np.array(table, np.uint16)
    if what == "mask":
        mk[200] |= np.uint64(1 << N)
    elif what == "cell":
        tb[8 * (N + 1) + 4] = n_ranks
    else:
        ml[:2] = (1 << 31)
    host = {k: np.full(max(c, 1) * np.dtype(DTYPES[k]).itemsize, 0xA5, np.uint8) for k, c in (("obs_rank", len(mk)), ("labels", P), ("perm_min", P), ("tail", tail_ranks))}
    rc = nat.lib().dcrx_assoc_permute(N, C_, len(mk), mk.ctypes.data, ml.ctypes.data, tb.ctypes.data, n_ranks, tail_ranks, P, seed,
                                      host["obs_rank"].ctypes.data, host["labels"].ctypes.data, host["perm_min"].ctypes.data,
                                      host["tail"].ctypes.data, None)
    assert rc == (E_UNSUPPORTED if what == "weight" else E_INVALID)
    assert all((v == 0xA5).all() for v in host.values())


@pytest.mark.parametrize("name", ["N33_census", "N63_two-sided", "N2_census", "past_a_slice"])
def test_the_device_entry_cuts_masks_and_never_reads_an_unused_cell(name):
    """Masks with bits at and above N, and a table whose unused cells hold 0xFFFF: the outputs are those of the cleaned input."""
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = au.constructed()[name]
    n1 = bin(C_).count("1")
    assert all(int(table[m * (N + 1) + k]) == 0xFFFF for m in range(N + 1) for k in range(N + 1) if k not in au.feasible(N, n1, m))
    rng = np.random.default_rng(5)
    dirt = rng.integers(0, 1 << (64 - N), size=len(masks), dtype=np.uint64) << np.uint64(N)
    dirty = np.asarray(masks, np.uint64) | dirt
    assert int((dirty >> np.uint64(N)).max()) > 0
    args = (dirty, mults, N, C_, table, n_ranks, tail_ranks, P, seed)
    want = au.expected_permute(*args, clean=True)
    au.assert_same(want, _want(name), "the contract of the cleaned input")
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    au.assert_same({k: outs[k].read() for k in au.OUTPUTS}, want, name)      # (read() holds the 64 guard bytes behind every output)


# ---- end to end ----

def _stage(tmp_path, kind, sub, **more):
    out = tmp_path / sub
    out.mkdir()
    text = au.tabulate_text() if kind == "tabulate" else au.public_text()
    (out / "in.tsv.gz").write_bytes(gzip.compress(text))
    (out / "cohort.tsv").write_bytes(au.phenotype_text())
    inp = {"command": "associate", "infile": str(out / "in.tsv.gz"), "phenotype": str(out / "cohort.tsv"), "case": "CMV+",
           "outpath": str(out) + os.sep, "prefix": "e_", "dontgzip": True, "permutations": 999, "write_null": True, "seed": 7}
    inp.update(more)
    return asc.run(inp)


@pytest.mark.parametrize("kind,alternative", [("tabulate", "greater"), ("public", "two-sided")])
def test_stage_on_the_device_writes_the_contracts_files(tmp_path, monkeypatch, kind, alternative):
    on_device = _stage(tmp_path, kind, "device", alternative=alternative, max_p="1/2")
    again = _stage(tmp_path, kind, "again", alternative=alternative, max_p="1/2")
    monkeypatch.setattr(nat, "assoc_permute", au.python_permute())
    over_contract = _stage(tmp_path, kind, "contract", alternative=alternative, max_p="1/2")
    for key in ("associate", "null"):
        a, b, c = (open(r[key], "rb").read() for r in (on_device, again, over_contract))
        assert a == c and a == b and len(a.split(b"\n")) > 3      # byte for byte the stage over the contract's; a second run the same
    au.assert_same(on_device["result"], over_contract["result"])
    identity, rows = au.identity_rows(kind)
    what = "clonotypes" if kind == "tabulate" else "reads"
    hand = au.hand_masks(what, 1)      # from the list of features, not from the files
    table, p_of_rank = au.rank_table(16, 8, alternative)
    null = au.expected_permute(hand, np.ones(len(hand), np.uint32), 16, au.HAND_CASE_MASK, table, len(p_of_rank),
                               sum(p <= Fraction(1, 2) for p in p_of_rank), 999, 7)
    want_main, want_null = au.stage_files(identity, rows, hand, 16, au.HAND_CASE_MASK, alternative, Fraction(1, 2), 999, null)
    assert open(on_device["associate"], "rb").read() == want_main and open(on_device["null"], "rb").read() == want_null
