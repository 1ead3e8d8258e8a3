"""The wide permutation null on the device (include/dcrx.h "association, wide"): both entries on every output cell against the
contract in plain Python (tests/assoc_wide_util.expected_permute_wide) over the constructed cases — every sample count around a
word's edge up to 1024, one case and one control, a census of 263 169 ranks with cells above 65 535, the edges of a slice and of
a block's relabelings at four, two and one relabeling a lane (read from the host build), ascending and shuffled popcount, popcount
0 and N, the last partial word, the 64-bit cells, multiplicities of 0, the extreme seeds —, agreement with the narrow entry up to
64 samples, outputs prefilled and guarded, two calls on one stream without a wait between them, the refusals with every output
byte left alone, what the device entry makes of masks and tables it cannot check, and the stage end to end over two tables."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import associate as asc
from tests import assoc_util as au
from tests import assoc_wide_util as awu

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2
GUARD = 64
DTYPES = {"obs_rank": np.uint32, "labels": np.uint64, "perm_min": np.uint32, "tail": np.uint64}


@functools.lru_cache(maxsize=None)
def _want(name):
    args = awu.constructed()[name]
    want = awu.expected_permute_wide(*args)
    awu.premise(name, args, want)
    for key in au.OUTPUTS:
        want[key].setflags(write=False)
    return want


def _counts(args):
    return {"obs_rank": len(args[0]), "labels": args[7] * awu.words_for(args[2]), "perm_min": args[7], "tail": args[6]}


class _Out:
    """An output array of exactly `count` entries with GUARD bytes behind it, 0xA5 all over before the call."""

    def __init__(self, dtype, count):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.bytes = self.count * self.dtype.itemsize
        self.buf = nat.DeviceBuffer.from_host(np.full(self.bytes + GUARD, 0xA5, np.uint8))
        self.ptr = self.buf.ptr

    def raw(self):
        return self.buf.to_host(np.uint8, self.bytes + GUARD)

    def read(self):
        raw = self.raw()
        assert (raw[self.bytes:] == 0xA5).all(), "written behind an output array"
        return raw[:self.bytes].view(self.dtype).copy()


def _outs(counts):
    return {k: _Out(DTYPES[k], counts[k]) for k in au.OUTPUTS}


def _inputs(args):
    masks, mults, N, cw, table = args[:5]
    return (nat.DeviceBuffer.from_host(np.ascontiguousarray(masks, np.uint64).reshape(-1) if len(masks) else np.zeros(1, np.uint64)),
            nat.DeviceBuffer.from_host(np.ascontiguousarray(mults, np.uint32) if len(mults) else np.zeros(1, np.uint32)),
            nat.DeviceBuffer.from_host(np.ascontiguousarray(table, np.uint32)))


def _launch(args, inputs, outs, stream=None):
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = args
    nat.assoc_permute_wide_device(N, cw, len(masks), inputs[0], inputs[1], inputs[2], n_ranks, tail_ranks, P, seed, outs["obs_rank"], outs["labels"],
                                  outs["perm_min"], outs["tail"], stream)


def _read(outs, args):
    got = {k: outs[k].read() for k in au.OUTPUTS}
    got["labels"] = got["labels"].reshape(args[7], awu.words_for(args[2]))
    return got


@pytest.mark.parametrize("name", awu.constructed_names())
def test_both_entries_against_the_contract(name):
    args = awu.constructed()[name]
    want = _want(name)
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = args
    got = nat.assoc_permute_wide(*args)
    awu.assert_same(got, want, (name, "host entry"))
    assert got["stats"] == want["stats"], name
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    awu.assert_same(_read(outs, args), want, (name, "device entry"))


@pytest.mark.parametrize("name", ["N2_census", "N63_two-sided", "N64_greater", "N64_census", "N64_one_case", "N64_one_control", "past_both",
                                  "three_of_one_mask_sum_to_2_32_less_1", "every_feature_is_the_case_mask", "seed_max"])
def test_up_to_64_samples_the_wide_entry_is_the_narrow_entry(name):
    masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed = au.constructed()[name]
    narrow = nat.assoc_permute(masks, mults, N, C_, table, n_ranks, tail_ranks, P, seed)
    wide = nat.assoc_permute_wide(masks.reshape(-1, 1), mults, N, np.array([C_], np.uint64), table.astype(np.uint32), n_ranks, tail_ranks, P, seed)
    assert wide["labels"].shape == (P, 1)
    awu.assert_same(wide, narrow, name)      # all four arrays, labels included
    assert wide["stats"] == narrow["stats"]


def test_a_large_then_a_small_call_on_one_stream_without_a_wait():
    big, small = "past_both", "tail_1"
    a_big, a_small = awu.constructed()[big], awu.constructed()[small]
    assert all(0 < _counts(a_small)[k] < _counts(a_big)[k] for k in au.OUTPUTS)      # the small call fits the large one's arrays
    stream = nat.Stream()
    in_big, in_small = _inputs(a_big), _inputs(a_small)
    first, second = _outs(_counts(a_big)), _outs(_counts(a_small))
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, second, stream.ptr)
    stream.synchronize()
    awu.assert_same(_read(first, a_big), _want(big), "the large call")
    awu.assert_same(_read(second, a_small), _want(small), "the small call behind it")
    # and the small call into the large one's arrays, behind a second large call: its cells in front, the large call's behind
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, first, stream.ptr)
    stream.synchronize()
    for k in au.OUTPUTS:
        n, both = _counts(a_small)[k], first[k].read()
        assert np.array_equal(both[:n], np.asarray(_want(small)[k]).astype(DTYPES[k]).reshape(-1)), k
        assert np.array_equal(both[n:], np.asarray(_want(big)[k]).astype(DTYPES[k]).reshape(-1)[n:]), k


REFUSED = [({"N": 1}, E_INVALID), ({"N": 1025}, E_INVALID), ({"C": 0}, E_INVALID), ({"C": (1 << 100) - 1}, E_INVALID),
           ({"n_ranks": 0, "tail": 0}, E_INVALID), ({"n_ranks": 101 * 101 + 1}, E_INVALID), ({"tail": 10 ** 6}, E_INVALID),
           ({"P": (1 << 20) + 1}, E_UNSUPPORTED), ({"F": 1 << 30}, E_UNSUPPORTED), ({"null": "mask"}, E_INVALID), ({"null": "tail"}, E_INVALID),
           ({"null": "cases"}, E_INVALID)]


@pytest.mark.parametrize("change,code", REFUSED)
def test_refusals_leave_every_output_byte_alone(change, code):
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = awu.constructed()["F1"]
    masks, mults = awu.seeded_rows(N, 257, 3), au.seeded_mults(257, 3)
    a = dict({"N": N, "C": awu.to_int(cw), "F": len(masks), "n_ranks": n_ranks, "tail": 5, "P": P}, **{k: v for k, v in change.items() if k != "null"})
    cases = awu.to_words(a["C"], 2)
    c_ptr = None if change.get("null") == "cases" else cases.ctypes.data
    L = nat.lib()
    # the device entry, on device arrays
    inputs, outs = _inputs((masks, mults, N, cw, table)), _outs({"obs_rank": len(masks), "labels": 2 * P, "perm_min": P, "tail": 5})
    d_mask = None if change.get("null") == "mask" else inputs[0].ptr
    d_tail = None if change.get("null") == "tail" else outs["tail"].ptr
    rc = L.dcrx_assoc_permute_wide_device(a["N"], c_ptr, a["F"], d_mask, inputs[1].ptr, inputs[2].ptr, a["n_ranks"], a["tail"], a["P"], seed,
                                          outs["obs_rank"].ptr, outs["labels"].ptr, outs["perm_min"].ptr, d_tail, None)
    assert rc == code, L.dcrx_last_error()
    nat.synchronize()
    assert all((outs[k].raw() == 0xA5).all() for k in au.OUTPUTS)
    # the host entry, on host arrays
    host = {k: np.full(max(c, 1) * np.dtype(DTYPES[k]).itemsize, 0xA5, np.uint8) for k, c in (("obs_rank", len(masks)), ("labels", 2 * P), ("perm_min", P), ("tail", 5))}
    mk, ml, tb = np.ascontiguousarray(masks, np.uint64), np.ascontiguousarray(mults, np.uint32), np.ascontiguousarray(table, np.uint32)
    rc = L.dcrx_assoc_permute_wide(a["N"], c_ptr, a["F"], None if change.get("null") == "mask" else mk.ctypes.data, ml.ctypes.data, tb.ctypes.data,
                                   a["n_ranks"], a["tail"], a["P"], seed, host["obs_rank"].ctypes.data, host["labels"].ctypes.data,
                                   host["perm_min"].ctypes.data, None if change.get("null") == "tail" else host["tail"].ctypes.data, None)
    assert rc == code, L.dcrx_last_error()
    assert all((v == 0xA5).all() for v in host.values())


@pytest.mark.parametrize("what", ["case bit", "mask", "cell", "weight"])
def test_what_the_host_entry_sees_in_the_arrays_is_refused_before_any_write(what):
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = awu.constructed()["N129_census"]
    mk, ml, tb, cases = np.array(masks, np.uint64), np.array(mults, np.uint32), np.array(table, np.uint32), np.array(cw, np.uint64)
    if what == "case bit":
        cases[2] |= np.uint64(2)
    elif what == "mask":
        mk[100, 2] |= np.uint64(1 << 1)
    elif what == "cell":
        tb[8 * (N + 1) + 4] = n_ranks
    else:
        ml[:2] = (1 << 31)
    host = {k: np.full(max(c, 1) * np.dtype(DTYPES[k]).itemsize, 0xA5, np.uint8) for k, c in (("obs_rank", len(mk)), ("labels", 3 * P), ("perm_min", P), ("tail", tail_ranks))}
    rc = nat.lib().dcrx_assoc_permute_wide(N, cases.ctypes.data, len(mk), mk.ctypes.data, ml.ctypes.data, tb.ctypes.data, n_ranks, tail_ranks, P, seed,
                                           host["obs_rank"].ctypes.data, host["labels"].ctypes.data, host["perm_min"].ctypes.data,
                                           host["tail"].ctypes.data, None)
    assert rc == (E_UNSUPPORTED if what == "weight" else E_INVALID)
    assert all((v == 0xA5).all() for v in host.values())


@pytest.mark.parametrize("name", ["N65_census", "N129_census", "N2_census", "N1023_census", "F1025"])
def test_the_device_entry_cuts_masks_and_never_reads_an_unused_cell(name):
    """Masks and a case mask with bits at and above N, and a table whose unused cells hold 0xFFFFFFFF: the outputs are those of
    the cleaned input."""
    masks, mults, N, cw, table, n_ranks, tail_ranks, P, seed = awu.constructed()[name]
    n1, W, spare = awu.to_int(cw).bit_count(), awu.words_for(N), 64 * awu.words_for(N) - N
    assert all(int(table[m * (N + 1) + k]) == 0xFFFFFFFF for m in range(0, N + 1, 7) for k in range(N + 1) if k not in au.feasible(N, n1, m))
    rng = np.random.default_rng(5)
    dirty = np.array(masks, np.uint64)
    dirty[:, W - 1] |= rng.integers(1, 1 << spare, size=len(masks), dtype=np.uint64) << np.uint64(64 - spare)
    cases = np.array(cw, np.uint64)
    cases[W - 1] |= np.uint64(1) << np.uint64(63)
    args = (dirty, mults, N, cases, table, n_ranks, tail_ranks, P, seed)
    want = awu.expected_permute_wide(*args, clean=True)
    awu.assert_same(want, _want(name), "the contract of the cleaned input")
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    awu.assert_same(_read(outs, args), want, name)      # (read() holds the 64 guard bytes behind every output)


# ---- end to end ----

def _stage(tmp_path, sub, **more):
    out = tmp_path / sub
    out.mkdir()
    (out / "a.tsv").write_bytes(awu.tabulate_text(awu.FIRST))
    (out / "b.tsv").write_bytes(awu.tabulate_text(awu.SECOND))
    (out / "cohort.tsv").write_bytes(awu.phenotype_text())
    inp = {"command": "associate", "infile": [str(out / "a.tsv"), str(out / "b.tsv")], "phenotype": str(out / "cohort.tsv"), "case": "CMV+",
           "outpath": str(out) + os.sep, "prefix": "e_", "dontgzip": True, "permutations": 999, "write_null": True, "seed": 7}
    inp.update(more)
    return asc.run(inp)


@pytest.mark.parametrize("alternative", ["greater", "two-sided"])
def test_stage_on_the_device_writes_the_contracts_files(tmp_path, monkeypatch, alternative):
    on_device = _stage(tmp_path, "device", alternative=alternative, max_p="1/2")
    monkeypatch.setattr(nat, "assoc_permute_wide", awu.python_permute_wide())
    over_contract = _stage(tmp_path, "contract", alternative=alternative, max_p="1/2")
    for key in ("associate", "null"):
        a, c = (open(r[key], "rb").read() for r in (on_device, over_contract))
        assert a == c and len(a.split(b"\n")) > 3      # byte for byte the stage over the contract's
    awu.assert_same(on_device["result"], over_contract["result"])
    identity, rows = awu.identity_rows()
    hand = awu.hand_masks()      # from the list of features, not from the files
    table, n_ranks, _ = awu.exact_table(70, 27, alternative)
    p_of_rank = sorted(set(au.fisher_table(70, 27, alternative).values()))
    null = awu.expected_permute_wide(awu.rows_of(hand, 2), np.ones(len(hand), np.uint32), 70, awu.HAND_CASE_MASK, table, n_ranks,
                                     sum(p <= Fraction(1, 2) for p in p_of_rank), 999, 7)
    want_main, want_null = au.stage_files(identity, rows, hand, 70, awu.HAND_CASE_MASK, alternative, Fraction(1, 2), 999, null)
    assert open(on_device["associate"], "rb").read() == want_main and open(on_device["null"], "rb").read() == want_null
