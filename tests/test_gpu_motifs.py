"""`motifs` through the HIP path: dcrx_cdr3_motifs and dcrx_cdr3_motifs_device against the contract written in Python
(mu.expected_motifs: sets of slices, every key sorted) — k, code, cs, cb, ge, sum, max, need and the statistics exactly — on
degenerate tables, background sizes around the 32- and 64-unit marks, a background in which every other unit takes no part, kept
lists one shorter than, as long as and one longer than a block (the size taken from the kernels' own constants), a selection that
takes a second level, thresholds in the first and the last bin, resamples one below, at and one above a chunk, `cap` below
`need`, a work space one byte short, a stream of the caller's, two seeds, one random table, and the sub-command end to end."""
import ctypes

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import pipeline
from decombinator_amd.match import spans
from tests import motif_util as mu
from tests import test_motifs as cpu

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _check(sample, background, ks=(2, 3, 4), trim=(3, 3), min_count=1, resamples=3, seed=1, cap=None, want=None):
    s_off, s_text = spans(list(sample))
    b_off, b_text = spans(list(background))
    got = nat.cdr3_motifs(s_off, s_text, b_off, b_text, ks, trim, min_count, resamples, seed, cap)
    want = mu.expected_motifs(list(sample), list(background), ks, trim, min_count, resamples, seed, cap) if want is None else want
    mu.assert_same(got, want)
    return got, want


def _pool():
    return mu.random_units(400, 21, 8, 14)


# ---- degenerate cases ----

def test_empty_sample_and_empty_background():
    got, _ = _check([], _pool()[:50], resamples=3)
    assert got["need"] == 0 and got["stats"]["background_take_part"] == 50
    got, _ = _check(_pool()[:20], [], resamples=0)
    assert got["need"] > 0 and int(got["cb"].sum()) == 0
    _check([], [], resamples=0)


def test_one_unit_all_but_one_and_all_of_the_background():
    pool = _pool()
    _check(pool[:1], pool[:40], resamples=9)
    _check(pool[:39], pool[:40], resamples=9)
    got, _ = _check(pool[:40], pool[40:80], resamples=9)      # n' = m': every resample is the whole background
    assert all(int(ge) == (9 if cb >= cs else 0) for ge, cb, cs in zip(got["ge"], got["cb"], got["cs"]))
    with pytest.raises(nat.DcrxError) as e:
        _check(pool[:41], pool[:40], resamples=1, want={})
    assert e.value.code == E_INVALID and "41" in str(e.value) and "40" in str(e.value)
    _check(pool[:41], pool[:40], resamples=0)


def test_every_unit_too_short_for_a_window():
    short = [u[:6] for u in _pool()[:60]]
    got, _ = _check(list(dict.fromkeys(short))[:20], list(dict.fromkeys(short)), resamples=2)
    assert got["need"] == 0 and got["stats"]["sample_take_part"] == 20


@pytest.mark.parametrize("R", [0, 1, 65])
def test_resample_counts(R):
    pool = _pool()
    _check(pool[:30], pool[10:200], resamples=R, seed=5)


def test_units_that_take_no_part_on_both_sides():
    pool = list(_pool()[:120])
    odd = [b"", b"A" * 33, b"CASsLGYEF", b"CAS*LGYEF", b"CASSLGYE1", b"\x00\xffAB"]
    background = [x for pair in zip(pool[:100], (odd * 17)[:100]) for x in pair]      # every other unit takes no part
    got, _ = _check(pool[90:120] + odd, background, resamples=7, seed=2)
    assert got["stats"]["background_take_part"] == 100 and got["stats"]["background_units"] == 200


@pytest.mark.parametrize("m", [31, 32, 33, 63, 64, 65])
def test_background_sizes_around_a_word(m):
    pool = _pool()
    _check(pool[100:100 + m // 2], pool[:m], resamples=5, seed=m)


# ---- the kept lists' blocks ----

@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_kept_list_around_a_block(delta):
    """A background of one repeated 2-mer: every kept unit adds onto one row.  n' one below a block (the second resample's list
    then starts in the last entry of a block of the flat list), a block, and a block and one."""
    n = mu.constant("BLOCK") + delta
    unit = b"XXXABXXX"
    got, _ = _check([unit] * n, [unit] * (2 * n + 3), ks=(2,), resamples=3)
    assert [int(x) for x in got["sum"]] == [3 * n] and [int(x) for x in got["max"]] == [n]


def test_many_rows_of_one_unit_each():
    letters = mu.AMINO
    units = [b"XXX" + bytes([letters[i // 400 % 20], letters[i // 20 % 20], letters[i % 20], letters[(7 * i) % 20]]) + b"XXX" for i in range(900)]
    got, _ = _check(units[:300], units, ks=(4,), resamples=4)
    assert got["need"] == 300 and all(int(c) == 1 for c in got["cb"])


# ---- the selection ----

def _threshold_bin(taking, n_take, seed, r, levels=1):
    keys = np.sort(mu.ru.sample_keys(seed, r, len(taking)))
    bits = 64 // mu.constant("LEVELS")
    threshold = int(keys[n_take])
    return threshold >> (64 - bits * levels), int((keys >> np.uint64(64 - bits * levels) == np.uint64(threshold >> (64 - bits * levels))).sum())


def test_selection_takes_a_second_level():
    """The threshold's bin of the first level holds more keys than are written out, at a background a little above BINS times
    CANDIDATES units."""
    m = mu.constant("BINS") * mu.constant("CANDIDATES") * 5 // 4
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 400, size=m)
    background = [b"XXX" + bytes([mu.AMINO[c // 20], mu.AMINO[c % 20]]) + b"XXX" for c in codes.tolist()]
    _bin, held = _threshold_bin(range(m), 1000, 6, 0)
    assert held > mu.constant("CANDIDATES")
    _bin2, held2 = _threshold_bin(range(m), 1000, 6, 0, levels=2)
    assert held2 <= mu.constant("CANDIDATES")
    _check(background[:1000], background, ks=(2,), min_count=5, resamples=1, seed=6)


def test_threshold_in_the_first_and_in_the_last_bin():
    pool = mu.random_units(2000, 12)
    assert _threshold_bin(range(2000), 1, 8, 0)[0] == 0
    assert _threshold_bin(range(2000), 1999, 8, 0)[0] == mu.constant("BINS") - 1
    _check(pool[:1], pool, ks=(2,), resamples=1, seed=8)
    _check(pool[:1999], pool, ks=(2,), min_count=40, resamples=1, seed=8)


# ---- the resample chunks ----

@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_resamples_around_a_chunk(delta):
    pool = _pool()
    chunk = mu.chunk_of(25)
    assert chunk == mu.constant("MAX_CHUNK")
    _check(pool[:25], pool[5:150], ks=(2, 3), resamples=chunk + delta, seed=3)


# ---- further cases ----

def test_cap_below_need():
    pool = _pool()
    whole = mu.expected_motifs(list(pool[:30]), list(pool[:100]), min_count=1, resamples=4)
    assert whole["need"] > 40
    got, want = _check(pool[:30], pool[:100], resamples=4, cap=40)
    assert got["need"] == whole["need"] and len(got["k"]) == 40
    for f in mu.FIELDS:
        assert [int(x) for x in got[f]] == [int(x) for x in whole[f][:40]]
    _check(pool[:30], pool[:100], resamples=4, cap=0)


def _device_call(sample, background, ks, trim, min_count, resamples, seed, stream=None, bufs=None, short=0):
    n, m = len(sample), len(background)
    if bufs is None:
        s_off, s_text = spans(list(sample))
        b_off, b_text = spans(list(background))
        work = nat.cdr3_motifs_work_bytes(n, m, resamples)
        assert work > 0
        cap = n * 90
        bufs = {"in": [nat.DeviceBuffer.from_host(np.frombuffer(x, np.uint8) if isinstance(x, bytes) else x) for x in (s_off, s_text, b_off, b_text)],
                "out": [nat.DeviceBuffer(8 * cap + 16) for _ in range(7)], "need": nat.DeviceBuffer(16),
                "stats": nat.DeviceBuffer(ctypes.sizeof(nat.Cdr3MotifStatsC)), "work": nat.DeviceBuffer(work), "work_bytes": work, "cap": cap}
    i, o = bufs["in"], bufs["out"]
    nat.cdr3_motifs_device(n, i[0], i[1], m, i[2], i[3], ks, trim, min_count, resamples, seed, bufs["cap"], *o, bufs["need"], bufs["stats"],
                           bufs["work"], bufs["work_bytes"] - short, None if stream is None else stream.ptr)
    return bufs


def _device_result(bufs):
    need = int(bufs["need"].to_host(np.uint64, 1)[0])
    rows = min(need, bufs["cap"])
    got = {name: b.to_host(dt, rows) for (name, dt), b in zip(nat.CDR3_MOTIF_OUTPUTS, bufs["out"])}
    st = bufs["stats"].to_host(np.uint64, len(nat.CDR3_MOTIF_STATS))
    got.update(need=need, stats={k: int(v) for k, v in zip(nat.CDR3_MOTIF_STATS, st)})
    return got


def test_device_primitive_twice_in_a_row_on_a_stream_of_the_callers():
    """Two calls on one stream with no synchronisation between them, the second with another seed into the same arrays and the
    same work space: what comes back is the second call's."""
    pool = _pool()
    sample, background = list(pool[:50]), list(pool[20:300])
    stream = nat.Stream()
    bufs = _device_call(sample, background, (2, 3, 4), (3, 3), 2, 70, 1, stream)
    _device_call(sample, background, (2, 3, 4), (3, 3), 2, 70, 2, stream, bufs)
    stream.synchronize()
    mu.assert_same(_device_result(bufs), mu.expected_motifs(sample, background, (2, 3, 4), (3, 3), 2, 70, 2))


def test_a_work_space_one_byte_short_is_refused_not_launched():
    pool = _pool()
    sample, background = list(pool[:10]), list(pool[:30])
    bufs = _device_call(sample, background, (2,), (3, 3), 1, 2, 1)
    nat.synchronize()
    before = _device_result(bufs)
    nat.check(nat.lib().dcrx_memset_device(bufs["need"].ptr, 0xAB, 8))
    with pytest.raises(nat.DcrxError) as e:
        _device_call(sample, background, (2,), (3, 3), 1, 2, 1, None, bufs, short=1)
    assert e.value.code == E_INVALID
    nat.synchronize()
    assert int(bufs["need"].to_host(np.uint64, 1)[0]) == 0xABABABABABABABAB      # nothing ran
    _device_call(sample, background, (2,), (3, 3), 1, 2, 1, None, bufs)
    nat.synchronize()
    mu.assert_same(_device_result(bufs), before)
    mu.assert_same(before, mu.expected_motifs(sample, background, (2,), (3, 3), 1, 2, 1))


def test_bad_settings_are_refused():
    s_off, s_text = spans([b"CASSLGYEF"])
    for kwargs in ({"trim": (17, 0)}, {"min_count": 0}, {"resamples": 65536}):
        with pytest.raises(nat.DcrxError) as e:
            nat.cdr3_motifs(s_off, s_text, s_off, s_text, **kwargs)
        assert e.value.code == E_INVALID
    assert nat.cdr3_motifs_work_bytes(1 << 30, 1, 1) == 0 and nat.cdr3_motifs_work_bytes(1, 1, 65536) == 0


def test_two_seeds():
    pool = _pool()
    sample, background = pool[:60], pool[30:400]
    first, _ = _check(sample, background, resamples=20, seed=1)
    other, _ = _check(sample, background, resamples=20, seed=2)
    again, _ = _check(sample, background, resamples=20, seed=1)
    assert [int(x) for x in first["sum"]] == [int(x) for x in again["sum"]] != [int(x) for x in other["sum"]]
    assert [int(x) for x in first["cs"]] == [int(x) for x in other["cs"]]


def test_random_table_of_5000_against_20000():
    pool = mu.random_units(23000, 31)
    got, _ = _check(pool[:5000], pool[3000:], min_count=3, resamples=64, seed=7)
    assert got["need"] > 1000 and got["stats"]["background_take_part"] == 20000


def test_sub_command_end_to_end(tmp_path):
    a, b, bg = (str(tmp_path / name) for name in ("A.clonotypes.tsv", "B.clonotypes.tsv", "naive.clonotypes.tsv"))
    mu.clonotype_file(a, cpu.SAMPLE_A, repeat_first=2)
    mu.clonotype_file(b, cpu.SAMPLE_B)
    mu.clonotype_file(bg, cpu.BACKGROUND, repeat_first=3)
    out = str(tmp_path) + "/"
    pipeline.main(["motifs", "-in", a, b, "-bg", bg, "-op", out, "-dz", "--resamples", "50", "--motif-min-count", "1", "--seed", "4"])
    for name, units in (("A", cpu.SAMPLE_A), ("B", cpu.SAMPLE_B)):
        lines = open(out + f"dcr_{name}.cdr3_motifs.tsv").read().split("\n")
        want = mu.expected_motifs(units, cpu.BACKGROUND, (2, 3, 4), (3, 3), 1, 50, 4)
        assert lines[0] == cpu.HEAD and lines[-1] == "" and lines[1:-1] == mu.expected_lines(want, 50)
