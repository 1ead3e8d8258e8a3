"""The rank-sum null on the device (include/dcrx.h "association, rank-sum"): both entries on every output cell against the
contract (tests/assoc_ranksum_util.expected_ranksum) over the constructed cases — every sample count around a word's seam, one
case and one control, the three alternatives, the edges of a block's slice and of its relabelings (read from the host build),
the kinds of feature, the extreme scales, offsets and multiplicities, a tail cell past 2^32, 0, 1 and 1024 edges, the extreme
seeds —, the relabelings against the presence null's, outputs prefilled and guarded, two calls on one stream without a wait
between them, the refusals with every output byte left alone, plane bits above N fed to the device entry, and the stage end to
end."""
import functools
import gzip
import os

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import associate as asc
from tests import assoc_ranksum_util as ru
from tests import assoc_util as au

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2
GUARD = 64
DTYPES = {"obs_score": np.uint32, "labels": np.uint64, "perm_max": np.uint32, "exceed": np.uint32, "tail": np.uint64}


@functools.lru_cache(maxsize=None)
def _want(name):
    args = ru.constructed()[name]
    want = ru.expected_ranksum(*args)
    ru.premise(name, args, want)
    for key in ru.OUTPUTS:
        want[key].setflags(write=False)
    return want


def _counts(args):
    return {"obs_score": len(args[0]), "labels": args[8], "perm_max": args[8], "exceed": len(args[0]), "tail": len(args[7])}


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
    return {k: _Out(DTYPES[k], counts[k]) for k in ru.OUTPUTS}


def _inputs(args):
    planes, off, sc, mults = args[:4]
    edges = args[7]
    return [nat.DeviceBuffer.from_host(np.ascontiguousarray(x, t).reshape(-1)) if len(x) else None
            for x, t in ((planes, np.uint64), (off, np.uint32), (sc, np.uint32), (mults, np.uint32), (edges, np.uint32))]


def _launch(args, inputs, outs, stream=None):
    planes, off, sc, mults, N, C_, alt, edges, P, seed = args
    nat.assoc_ranksum_device(N, C_, alt, len(planes), inputs[0], inputs[1], inputs[2], inputs[3], len(edges), inputs[4], P, seed,
                             outs["obs_score"], outs["labels"], outs["perm_max"], outs["exceed"], outs["tail"], stream)


@pytest.mark.parametrize("name", ru.constructed_names())
def test_both_entries_against_the_contract(name):
    args = ru.constructed()[name]
    want = _want(name)
    planes, off, sc, mults, N, C_, alt, edges, P, seed = args
    got = nat.assoc_ranksum(*args)
    ru.assert_same(got, want, (name, "host entry"))
    assert got["stats"] == want["stats"], name
    n1 = bin(C_).count("1")
    assert all(bin(int(x)).count("1") == n1 and int(x) >> N == 0 for x in got["labels"])
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    ru.assert_same({k: outs[k].read() for k in ru.OUTPUTS}, want, (name, "device entry"))


@pytest.mark.parametrize("name", ["N2_greater", "N33_less", "N64_two-sided", "N64_one_case", "seed_0", "seed_max"])
def test_the_relabelings_are_the_presence_nulls(name):
    planes, off, sc, mults, N, C_, alt, edges, P, seed = ru.constructed()[name]
    table, n_ranks = au.census_table(N, bin(C_).count("1"))
    presence = nat.assoc_permute(np.zeros(1, np.uint64), np.ones(1, np.uint32), N, C_, table, n_ranks, 0, P, seed)
    assert np.array_equal(nat.assoc_ranksum(*ru.constructed()[name])["labels"], presence["labels"]) and P > 0


def test_a_large_then_a_small_call_on_one_stream_without_a_wait():
    big, small = "past_both", "E1"
    a_big, a_small = ru.constructed()[big], ru.constructed()[small]
    assert all(0 < _counts(a_small)[k] < _counts(a_big)[k] for k in ru.OUTPUTS)      # the small call fits the large one's arrays
    stream = nat.Stream()
    in_big, in_small = _inputs(a_big), _inputs(a_small)
    first, second = _outs(_counts(a_big)), _outs(_counts(a_small))
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, second, stream.ptr)
    stream.synchronize()
    ru.assert_same({k: first[k].read() for k in ru.OUTPUTS}, _want(big), "the large call")
    ru.assert_same({k: second[k].read() for k in ru.OUTPUTS}, _want(small), "the small call behind it")
    # and the small call into the large one's arrays, behind a second large call: its cells in front, the large call's behind
    _launch(a_big, in_big, first, stream.ptr)
    _launch(a_small, in_small, first, stream.ptr)
    stream.synchronize()
    for k in ru.OUTPUTS:
        n, both = _counts(a_small)[k], first[k].read()
        assert np.array_equal(both[:n], np.asarray(_want(small)[k]).astype(DTYPES[k])), k
        assert np.array_equal(both[n:], np.asarray(_want(big)[k]).astype(DTYPES[k])[n:]), k


REFUSED = [({"N": 1, "C": 1}, E_INVALID), ({"N": 65}, E_INVALID), ({"C": 0}, E_INVALID), ({"C": 0xFFFF}, E_INVALID), ({"C": 1 << 16}, E_INVALID),
           ({"alt": 3}, E_INVALID), ({"E": 1025}, E_INVALID), ({"P": (1 << 20) + 1}, E_UNSUPPORTED), ({"F": 1 << 30}, E_UNSUPPORTED),
           ({"null": "plane"}, E_INVALID), ({"null": "scale"}, E_INVALID), ({"null": "edges"}, E_INVALID), ({"null": "tail"}, E_INVALID),
           ({"null": "exceed"}, E_INVALID), ({"null": "labels"}, E_INVALID)]


def _call(entry, a, seed, ins, outs, null):
    def ptr(name, p):
        return None if null == name else p
    return entry(a["N"], a["C"], a["alt"], a["F"], ptr("plane", ins[0]), ins[1], ptr("scale", ins[2]), ins[3], a["E"], ptr("edges", ins[4]), a["P"],
                 seed, outs["obs_score"], ptr("labels", outs["labels"]), outs["perm_max"], ptr("exceed", outs["exceed"]), ptr("tail", outs["tail"]), None)


@pytest.mark.parametrize("change,code", REFUSED)
def test_refusals_leave_every_output_byte_alone(change, code):
    planes, off, sc, mults, N, C_, alt, edges, P, seed = ru.constructed()["F257"]
    a = dict({"N": N, "C": C_, "alt": alt, "F": len(planes), "E": len(edges), "P": P}, **{k: v for k, v in change.items() if k != "null"})
    L = nat.lib()
    counts = _counts((planes, off, sc, mults, N, C_, alt, edges, P, seed))
    inputs, outs = _inputs((planes, off, sc, mults, N, C_, alt, edges)), _outs(counts)
    rc = _call(L.dcrx_assoc_ranksum_device, a, seed, [b.ptr for b in inputs], {k: v.ptr for k, v in outs.items()}, change.get("null"))
    assert rc == code, L.dcrx_last_error()
    nat.synchronize()
    assert all((outs[k].raw() == 0xA5).all() for k in ru.OUTPUTS)
    host = {k: np.full(max(c, 1) * np.dtype(DTYPES[k]).itemsize, 0xA5, np.uint8) for k, c in counts.items()}
    arrays = [np.ascontiguousarray(x, t) for x, t in ((planes, np.uint64), (off, np.uint32), (sc, np.uint32), (mults, np.uint32), (edges, np.uint32))]
    rc = _call(L.dcrx_assoc_ranksum, a, seed, [x.ctypes.data for x in arrays], {k: v.ctypes.data for k, v in host.items()}, change.get("null"))
    assert rc == code, L.dcrx_last_error()
    assert all((v == 0xA5).all() for v in host.values())


@pytest.mark.parametrize("what", ["plane", "edges", "weight"])
def test_what_the_host_entry_sees_in_the_arrays_is_refused_before_any_write(what):
    planes, off, sc, mults, N, C_, alt, edges, P, seed = ru.constructed()["F257"]
    pl, ml, ed = np.array(planes, np.uint64), np.array(mults, np.uint32), np.array(edges, np.uint32)
    assert len(ed) > 2
    if what == "plane":
        pl[200, 3] |= np.uint64(1 << N)
    elif what == "edges":
        ed[2] = ed[1]
    else:
        ml[:2] = (1 << 31)
    with pytest.raises(nat.DcrxError) as e:
        nat.assoc_ranksum(pl, off, sc, ml, N, C_, alt, ed, P, seed)
    assert e.value.code == (E_UNSUPPORTED if what == "weight" else E_INVALID)


@pytest.mark.parametrize("name", ["N33_less", "N63_two-sided", "N2_greater", "past_a_slice"])
def test_the_device_entry_cuts_plane_bits_at_and_above_the_sample_count(name):
    planes, off, sc, mults, N, C_, alt, edges, P, seed = ru.constructed()[name]
    rng = np.random.default_rng(5)
    dirt = rng.integers(0, 1 << (64 - N), size=planes.shape, dtype=np.uint64) << np.uint64(N)
    dirty = np.asarray(planes, np.uint64) | dirt
    assert int((dirty >> np.uint64(N)).max()) > 0
    args = (dirty, off, sc, mults, N, C_, alt, edges, P, seed)
    want = ru.expected_ranksum(*args, clean=True)
    ru.assert_same(want, _want(name), "the contract of the cleaned input")
    inputs, outs = _inputs(args), _outs(_counts(args))
    _launch(args, inputs, outs)
    nat.synchronize()
    ru.assert_same({k: outs[k].read() for k in ru.OUTPUTS}, want, name)      # (read() holds the 64 guard bytes behind every output)


# ---- end to end ----

def _stage(tmp_path, kind, sub, **more):
    out = tmp_path / sub
    out.mkdir()
    text = ru.tabulate_text() if kind == "tabulate" else ru.public_text()
    (out / "in.tsv.gz").write_bytes(gzip.compress(text))
    (out / "cohort.tsv").write_bytes(au.phenotype_text())
    inp = {"command": "associate", "infile": str(out / "in.tsv.gz"), "phenotype": str(out / "cohort.tsv"), "case": "CMV+", "test": "rank-sum",
           "outpath": str(out) + os.sep, "prefix": "e_", "dontgzip": True, "permutations": 999, "write_null": True, "seed": 7}
    inp.update(more)
    return asc.run(inp)


@pytest.mark.parametrize("kind,alternative", [("tabulate", "greater"), ("public", "two-sided")])
def test_stage_on_the_device_writes_the_contracts_files(tmp_path, monkeypatch, kind, alternative):
    on_device = _stage(tmp_path, kind, "device", alternative=alternative)
    again = _stage(tmp_path, kind, "again", alternative=alternative)
    monkeypatch.setattr(nat, "assoc_ranksum", ru.python_ranksum())
    over_contract = _stage(tmp_path, kind, "contract", alternative=alternative)
    for key in ("associate", "null"):
        a, b, c = (open(r[key], "rb").read() for r in (on_device, again, over_contract))
        assert a == c and a == b and len(a.split(b"\n")) > 3      # byte for byte the stage over the contract's; a second run the same
    ru.assert_same(on_device["result"], over_contract["result"])
    identity, rows = ru.identity_rows(kind)
    x_rows = ru.hand_values("clonotypes" if kind == "tabulate" else "reads", 1)      # from the list of features, not from the files
    null = ru.hand_null(x_rows, alternative, 999, 7)
    want_main, want_null, _, _ = ru.stage_files(identity, rows, x_rows, 16, au.HAND_CASE_MASK, alternative, 999, null)
    assert open(on_device["associate"], "rb").read() == want_main and open(on_device["null"], "rb").read() == want_null
