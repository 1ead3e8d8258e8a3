"""What the motif tests share (`motifs`; include/dcrx.h "motifs"): the contract as Python that shares no method with the
kernels — a unit's motifs as a set of slices, every key of a resample computed with numpy uint64 arithmetic and sorted in
full, counts taken over the kept units' sets —, the random tables, the stand-in for the native call, the text a result is
written as, and the host build of the shared header (tests/host_motif)."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

from decombinator_amd import _native as nat
from tests import rarefy_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host_motif", "build", "libmotif_host.so")
FIELDS = ("k", "code", "cs", "cb", "ge", "sum", "max")
AMINO = b"ACDEFGHIKLMNPQRSTVWY"


class Invalid(Exception):
    """What the contract answers with DCRX_E_INVALID."""


# ---- the contract ----

def takes_part(unit: bytes) -> bool:
    return 1 <= len(unit) <= 32 and all(65 <= b <= 90 for b in unit)


def motif_set(unit: bytes, ks, trim) -> set:
    """The (k, letters) a unit that takes part contains: the slices of its windows, as a set."""
    N, C_ = trim
    return {(k, unit[p:p + k]) for k in ks for p in range(N, len(unit) - C_ - k + 1)}


def code_of(letters: bytes) -> int:
    c = 0
    for b in letters:
        c = c * 26 + (b - 65)
    return c


def kept_units(taking, n_take: int, seed: int, r: int) -> np.ndarray:
    """The background indices resample r keeps: `taking` are the indices b of the units that take part; the n_take of them
    whose key(seed, r, b) are smallest, by a full sort."""
    taking = np.asarray(taking, dtype=np.int64)
    if n_take == len(taking):
        return taking
    last = int(taking.max()) + 1 if len(taking) else 0
    keys = ru.sample_keys(int(seed), int(r), last)[taking]
    return taking[np.argsort(keys, kind="stable")[:n_take]]


def census(units) -> tuple:
    """(take part, out of reach, not letters)."""
    reach = [u for u in units if 1 <= len(u) <= 32]
    take = sum(takes_part(u) for u in reach)
    return take, len(units) - len(reach), len(reach) - take


def expected_motifs(sample, background, ks=(2, 3, 4), trim=(3, 3), min_count=3, resamples=1000, seed=1, cap=None) -> dict:
    """What nat.cdr3_motifs gives for the units `sample` and `background` (lists of bytes, taken as given)."""
    ks = sorted(set(int(k) for k in ks))
    if not ks or any(k not in (2, 3, 4) for k in ks) or max(trim) > 16 or min(trim) < 0 or min_count < 1 or not 0 <= resamples <= 65535:
        raise Invalid("settings")
    s_take, s_far, s_odd = census(sample)
    b_take, b_far, b_odd = census(background)
    if resamples and s_take > b_take:
        raise Invalid(f"{s_take} > {b_take}")
    cs = {}
    for u in sample:
        if takes_part(u):
            for mo in motif_set(u, ks, trim):
                cs[mo] = cs.get(mo, 0) + 1
    reported = sorted(mo for mo, c in cs.items() if c >= min_count)      # (k, letters) ascending
    row = {mo: i for i, mo in enumerate(reported)}
    taking = [b for b, u in enumerate(background) if takes_part(u)]
    # per background unit that takes part, the reported rows it contains (from its set): flat, with the unit of every entry
    flat, owner = [], []
    for b in taking:
        rows = [row[mo] for mo in motif_set(background[b], ks, trim) if mo in row]
        flat += rows
        owner += [b] * len(rows)
    flat, owner = np.array(flat, dtype=np.int64), np.array(owner, dtype=np.int64)
    P = len(reported)
    cb = np.bincount(flat, minlength=P)
    want = np.array([cs[mo] for mo in reported], dtype=np.int64)
    ge, total, mx = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    kept_counts = []
    for r in range(resamples if P and s_take else 0):
        kept = kept_units(taking, s_take, seed, r)
        kept_counts.append(len(kept))
        mask = np.zeros(len(background) + 1, dtype=bool)
        mask[kept] = True
        c = np.bincount(flat[mask[owner]], minlength=P)
        ge += c >= want
        total += c
        mx = np.maximum(mx, c)
    got = P if cap is None else min(P, int(cap))
    out = {"k": np.array([mo[0] for mo in reported], np.uint32)[:got], "code": np.array([code_of(mo[1]) for mo in reported], np.uint32)[:got],
           "cs": want.astype(np.uint32)[:got], "cb": cb.astype(np.uint32)[:got], "ge": ge.astype(np.uint32)[:got],
           "sum": total.astype(np.uint64)[:got], "max": mx.astype(np.uint32)[:got], "need": P, "kept_counts": kept_counts,
           "letters": [mo[1].decode() for mo in reported][:got]}
    out["stats"] = dict(zip(nat.CDR3_MOTIF_STATS, (len(sample), s_take, s_far, s_odd, len(background), b_take, b_far, b_odd, len(cs), P)))
    return out


def assert_same(got: dict, want: dict):
    """Every field, `need` and the statistics, exactly."""
    for f in FIELDS:
        assert [int(x) for x in got[f]] == [int(x) for x in want[f]], f
    assert int(got["need"]) == int(want["need"])
    assert got["stats"] == want["stats"]


def native_stand_in(s_off, s_text, b_off, b_text, ks, trim, min_count, resamples, seed, cap=None) -> dict:
    """nat.cdr3_motifs' signature over the contract (for the stage tests, which run without a GPU)."""
    cut = lambda off, text: [bytes(text[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    return expected_motifs(cut(s_off, s_text), cut(b_off, b_text), ks, trim, min_count, resamples, seed, cap)


def ratio(num: int, den: int) -> str:
    return format(float(Fraction(num, den)), ".6f") if den else "nan"


def expected_lines(result: dict, resamples: int) -> list:
    """The file's lines (without the header) from a contract result: sorted by (ge, -cs, k, letters)."""
    rows = sorted(zip([int(x) for x in result["ge"]], [-int(x) for x in result["cs"]], [int(x) for x in result["k"]], result["letters"],
                      [int(x) for x in result["cb"]], [int(x) for x in result["sum"]], [int(x) for x in result["max"]]))
    R = resamples
    return ["\t".join([mo, str(k), str(-ncs), str(cb), str(R), str(ge), str(total), str(mx), ratio(total, R), ratio(-ncs * R, total),
                       ratio(ge + 1, R + 1)]) for ge, ncs, k, mo, cb, total, mx in rows]


# ---- tables ----

@functools.lru_cache(maxsize=8)
def random_units(count: int, seed: int, lo: int = 11, hi: int = 17) -> tuple:
    """`count` distinct random units of lo .. hi amino-acid letters (read only: shared between the tests that need them)."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < count:
        u = bytes(rng.choice(np.frombuffer(AMINO, np.uint8), size=int(rng.integers(lo, hi + 1))).tolist())
        if u not in seen:
            seen.add(u)
            out.append(u)
    return tuple(out)


def planted(units, motif: bytes, at: int, how_many: int) -> list:
    """The first `how_many` units with `motif` written from position `at` (0-based)."""
    return [u[:at] + motif + u[at + len(motif):] if i < how_many else u for i, u in enumerate(units)]


def clonotype_file(path, units, repeat_first: int = 0):
    """A .clonotypes.tsv of one row per unit (and the first `repeat_first` units once more under another V: one unit still)."""
    from decombinator_amd.overlap import HEADER
    rows = [b"\t".join([b"TRBV1", b"TRBJ1", u, b"1"] + [b"x"] * (HEADER.count(b"\t") - 3)) for u in units]
    rows += [b"\t".join([b"TRBV2", b"TRBJ1", u, b"2"] + [b"x"] * (HEADER.count(b"\t") - 3)) for u in units[:repeat_first]]
    with open(path, "wb") as fh:
        fh.write(HEADER + b"\n" + b"\n".join(rows) + (b"\n" if rows else b""))


# ---- the host build of the shared header ----

_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_motif")])
        _host = C.CDLL(HOST_LIB)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        for name in ("block", "bins", "levels", "candidates", "motifs", "max_windows", "max_chunk"):
            getattr(_host, "motif_host_" + name).restype = u32
        _host.motif_host_chunk_of.restype, _host.motif_host_chunk_of.argtypes = u32, [u64]
        _host.motif_host_digit.restype, _host.motif_host_digit.argtypes = u32, [u64, u32]
        _host.motif_host_prefix.restype, _host.motif_host_prefix.argtypes = u64, [u64, u32]
        _host.motif_host_window_count.restype, _host.motif_host_window_count.argtypes = u32, [u32, u32, u32, u32]
        _host.motif_host_takes_part.restype, _host.motif_host_takes_part.argtypes = C.c_int, [C.c_char_p, u64]
        _host.motif_host_code_at.restype, _host.motif_host_code_at.argtypes = u32, [C.c_char_p, u64, u32, u32]
        _host.motif_host_motif_id.restype, _host.motif_host_motif_id.argtypes = u32, [u32, u32]
        _host.motif_host_id_k.restype, _host.motif_host_id_k.argtypes = u32, [u32]
        _host.motif_host_id_code.restype, _host.motif_host_id_code.argtypes = u32, [u32]
        _host.motif_host_unit_motifs.restype, _host.motif_host_unit_motifs.argtypes = C.c_int, [C.c_char_p, u64, u32, u32, u32, vp]
    return _host


def constant(name: str) -> int:
    """BLOCK, BINS, LEVELS, CANDIDATES, MOTIFS, MAX_WINDOWS, MAX_CHUNK as the kernels have them."""
    return int(getattr(host_lib(), "motif_host_" + name.lower())())


def chunk_of(n: int) -> int:
    """The resamples of one chunk for n sample units, as the work space is carved."""
    return int(host_lib().motif_host_chunk_of(int(n)))


def host_unit_motifs(unit: bytes, trim, k: int):
    """A unit's motif numbers of one k from the shared header, in window order (None: the unit takes no part)."""
    out = np.zeros(constant("MAX_WINDOWS"), np.uint32)
    n = host_lib().motif_host_unit_motifs(unit, len(unit), int(trim[0]), int(trim[1]), int(k), out.ctypes.data)
    return None if n < 0 else [int(x) for x in out[:n]]
