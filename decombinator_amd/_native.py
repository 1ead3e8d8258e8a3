"""ctypes binding of libdcrx.so (include/dcrx.h, include/dcrx_synth.h).

The HIP library IS the product: there is no Python or CPU implementation of the
hot path behind this module.  Importing it fails loudly when the shared object
has not been built (`python -c "import __graft_entry__ as g; g.build()"` or
`make -C decombinator_amd/csrc`), and every decombine call raises DcrxError
when no GPU is present.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCRX_LIB_PATH: developer override for A/B builds of the same library (never a different backend)
LIB_PATH = os.environ.get("DCRX_LIB_PATH") or os.path.join(_HERE, "csrc", "libdcrx.so")

N_COUNTERS = 32
ABI_VERSION = 5

# enum dcrx_counter order; the strings are the reference's Counter keys
# (reference decombine.py:598 and the increments cited in include/dcrx_codes.h)
COUNTER_NAMES = [
    "multiple_v_matches", "verr2", "foundv1notv2", "verr1", "foundv2notv1",
    "no_vtags_found", "multiple_j_matches", "jerr2", "foundj1notj2", "jerr1",
    "no_j_assigned", "dcrfilter_intertagN", "dcrfilter_toolong_intertag",
    "dcrfilter_imposs_deletion", "dcrfilter_tag_overlap", "VJ_assignment_failed",
    "v_del_failed_tag_at_end", "v_del_failed", "j_del_failed", "vj_count",
    "read_count", "foundj2notj1", "frame_forward",
]

DEVICE_ERRORS = 31      # DCRX_C_DEVICE_ERRORS (not a reference counter)

STATUS_NAMES = [
    "OK", "V_MULTI", "V_WALK_FAIL_AT_END", "V_WALK_FAIL", "V_HALF1_EXHAUSTED", "V_HALF2_EXHAUSTED",
    "V_NONE", "J_MULTI", "J_WALK_FAIL", "J_HALF1_EXHAUSTED", "J_HALF2_EXHAUSTED", "J_NONE",
    "F_INTERTAG_N", "F_TOOLONG", "F_IMPOSS_DEL", "F_OVERLAP",
]

ORIENTATIONS = {"reverse": 0, "forward": 1, "both": 2}
F_FORCE_SLOW_READER = 1
F_PROFILE_SCAN_ONLY = 2
F_ONE_BASE_SCAN = 4
F_V1_KERNELS = 64        # the three-launch form even where the v2 kernel applies
F_V2_NO_LEAN_RESCUE = 8192   # A/B and tests: event entries go to the general form at once (no lean rescue kernel)
F_V2_LEAN_SERIAL = 32768     # A/B: the finishing roles as launches of their own, one after the other (default: roles of one launch)
F_V2_NO_FUSE = 131072       # A/B: no tail inside the scan kernel
F_V2_SIDE_STREAMS = 65536    # A/B: round 3's shape, the tail kernel and the X pass on side streams beside the rescue kernel


def F_V2_SHAPE(k):
    """v2 kernel launch shape (A/B): 1 = one read per lane, two blocks per CU; 2 = two reads per lane; 3 = one read, one block."""
    return int(k) << 8

F_PROFILE_LIST_SCAN_ONLY = 8
F_LIST_RESCUE = 16      # rescue queue through the list kernel even when the pair form applies

RECORD_DTYPE = np.dtype([
    ("v", "<u2"), ("j", "<u2"), ("v_start", "<u2"), ("j_end", "<u2"),
    ("ins_start", "<u2"), ("ins_len", "<u2"), ("vdel", "u1"), ("jdel", "u1"),
    ("status", "u1"), ("frame", "u1"),
])
assert RECORD_DTYPE.itemsize == 16


class DcrxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dcrx error {code}: {msg}")
        self.code = code


class TagSetC(C.Structure):
    _fields_ = [
        ("n_v", C.c_uint32), ("v_tags", C.POINTER(C.c_char_p)), ("v_jumps", C.POINTER(C.c_int32)),
        ("v_regions", C.POINTER(C.c_char_p)),
        ("n_j", C.c_uint32), ("j_tags", C.POINTER(C.c_char_p)), ("j_jumps", C.POINTER(C.c_int32)),
        ("j_regions", C.POINTER(C.c_char_p)),
        ("v_half_split", C.c_int32), ("j_half_split", C.c_int32),
    ]


class TablesInfoC(C.Structure):
    _fields_ = [
        ("n_v", C.c_uint32), ("n_j", C.c_uint32), ("n_states", C.c_uint32), ("dfa_bytes", C.c_uint32),
        ("n_keywords", C.c_uint32 * 6), ("max_tag_len", C.c_uint32), ("tables_in_lds", C.c_uint32),
        ("equal_len_per_automaton", C.c_uint32), ("pair_scan_bytes", C.c_uint32),
        ("v2_tables", C.c_uint32), ("v2_states", C.c_uint32 * 2), ("v2_scan_bytes", C.c_uint32 * 2), ("max_read_len", C.c_uint32),
    ]


class TupleLayoutC(C.Structure):
    _fields_ = [("w_v", C.c_uint8), ("w_j", C.c_uint8), ("w_vdel", C.c_uint8), ("w_jdel", C.c_uint8), ("w_pos", C.c_uint8),
                ("bits", C.c_uint8), ("bytes", C.c_uint8), ("reserved", C.c_uint8), ("max_read_len", C.c_uint32)]


class CfgC(C.Structure):
    _fields_ = [("orientation", C.c_int32), ("allow_ns", C.c_int32), ("lenthreshold", C.c_int32),
                ("flags", C.c_uint32)]


class BatchC(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("packed", C.c_void_p), ("stride", C.c_uint32), ("read_len", C.c_uint32),
        ("lens", C.c_void_p), ("n_exc", C.c_uint64), ("exc_read", C.c_void_p), ("exc_pos", C.c_void_p),
        ("exc_chr", C.c_void_p),
    ]


class FastqBatchC(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("text", C.c_void_p), ("text_bytes", C.c_uint64),
        ("name_off", C.c_void_p), ("name_len", C.c_void_p), ("seq_off", C.c_void_p), ("seq_len", C.c_void_p),
        ("qual_off", C.c_void_p), ("qual_len", C.c_void_p),
    ]


class SpansC(C.Structure):
    _fields_ = [("text", C.c_void_p), ("start", C.c_void_p), ("len", C.c_void_p)]


_collapse_tls = threading.local()      # per thread: the row buffer of its last collapse_front call


class CollapseCfgC(C.Structure):
    _fields_ = [("oligo", C.c_int32), ("allow_ns", C.c_int32), ("lenthreshold", C.c_int32), ("min_bc_q", C.c_double),
                ("bc_q_below_min", C.c_double), ("avg_q_threshold", C.c_double), ("field_sep", C.c_char * 8)]


COLLAPSE_ROW_DTYPE = np.dtype([("b1start", "<i2"), ("b1end", "<i2"), ("b2start", "<i2"), ("b2end", "<i2"), ("status", "u1"),
                               ("barcode_len", "u1"), ("barcode_qual_len", "u1"), ("pad", "u1"), ("barcode", "S24"), ("barcode_qual", "S24")])
assert COLLAPSE_ROW_DTYPE.itemsize == 60
COLLAPSE_OLIGOS = {"m13": 0, "i8": 1, "i8_single": 2, "nebio": 3, "takara": 4}
COLLAPSE_COUNTERS = [
    "readdata_input_dcrs", "getbarcode_fail_N", "getbarcode_fail_nospacerfound", "getbarcode_fail_not2spacersfound",
    "getbarcode_fail_n1tooshort", "getbarcode_fail_n1toolong", "getbarcode_fail_n2pastend", "getbarcode_pass_exactmatch",
    "getbarcode_pass_regexmatch", "getbarcode_pass_fuzzymatch_rightlen", "getbarcode_pass_fuzzymatch_short",
    "getbarcode_pass_fuzzymatch_long", "getbarcode_pass_other", "readdata_fail_no_bclocs", "readdata_short_barcode",
    "readdata_long_barcode", "readdata_fail_low_barcode_quality", "readdata_fail_overlong_intertag_seq", "readdata_success",
]
CF_OK, CF_NO_BCLOCS, CF_LOW_QUALITY, CF_OVERLONG, CF_DEFER = 0, 1, 2, 3, 255


def spacer_search(seq: str, spacer: str):
    """dcrx_spacer_search: ([(start, length), ...] of every match, kind) — kind 0 verbatim, 1 substitutions, 2 indel."""
    sb, pb = seq.encode("latin-1", "replace"), spacer.encode("latin-1", "replace")
    cap = len(sb) + 1
    starts = np.zeros(cap, dtype=np.int32)
    lens = np.zeros(cap, dtype=np.int32)
    kind = C.c_int32(0)
    n = check(lib().dcrx_spacer_search(sb, len(sb), pb, len(pb), starts.ctypes.data, lens.ctypes.data, cap, C.byref(kind)))
    return [(int(starts[k]), int(lens[k])) for k in range(min(n, cap))], int(kind.value)


def collapse_front(text: bytes, oligo: str, allow_ns: bool, lenthreshold: int, quality_parameters, field_sep: str = ", ", n_threads: int = 0):
    """dcrx_collapse_front over `.n12` text: (rows as COLLAPSE_ROW_DTYPE, row offsets (n + 1), counters uint64[len(COLLAPSE_COUNTERS)])."""
    cfg = CollapseCfgC()
    cfg.oligo = COLLAPSE_OLIGOS[oligo.lower()]
    cfg.allow_ns, cfg.lenthreshold = int(bool(allow_ns)), int(lenthreshold)
    cfg.min_bc_q, cfg.bc_q_below_min, cfg.avg_q_threshold = (float(x) for x in quality_parameters)
    cfg.field_sep = field_sep.encode("ascii")
    buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
    scratch = np.zeros(len(COLLAPSE_COUNTERS), dtype=np.uint64)
    n = check(lib().dcrx_collapse_front(buf.ctypes.data, len(text), C.byref(cfg), None, 0, None, scratch.ctypes.data, 0))      # sizing call
    # (the per-row records of a call are written once and the pages behind a fresh allocation cost more than the rows themselves:
    # the buffer of the last call is kept and handed out again when the caller has let go of it)
    # (per thread: two threads never share a buffer, and a thread hands its own out again only when nothing else refers to it)
    held = getattr(_collapse_tls, "buf", None)
    if held is None or len(held) < n or sys.getrefcount(held) > 3:
        held = np.empty(max(n, 1), dtype=COLLAPSE_ROW_DTYPE)
        _collapse_tls.buf = held
    rows = held
    del held
    offs = np.empty(n + 1, dtype=np.uint64)
    cnt = np.zeros(len(COLLAPSE_COUNTERS), dtype=np.uint64)
    check(lib().dcrx_collapse_front(buf.ctypes.data, len(text), C.byref(cfg), rows.ctypes.data, n, offs.ctypes.data, cnt.ctypes.data, int(n_threads)))
    return rows[:n], offs, cnt


# ---- stage 2 of collapse: UMI neighbour search (dcrx_umi.hip), grouping and counting (dcrx_collapse_back.cpp) ----

UMI_MAX_LEN, UMI_MAX_SYMBOLS, UMI_TILE, UMI_REC_WORDS, UMI_TILE_WORDS = 24, 8, 256, 16, 8
GRP_COUNTERS = ["readdata_barcode_dcretc_keys", "number_input_unique_dcrs", "number_input_total_dcrs", "multi_tcr_barcodes",
                "multi_tcr_barcode_reads"]


def text_and_offsets(strings):
    """(bytes, uint64 offsets of len + 1) of a list of str / bytes, or the pair itself when given one."""
    if isinstance(strings, tuple) and len(strings) == 2 and isinstance(strings[0], (bytes, bytearray)):
        return bytes(strings[0]), np.ascontiguousarray(strings[1], dtype=np.uint64)
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return b"".join(bs), off


def _buf(text: bytes):
    return np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)


def umi_encode(umis):
    """dcrx_umi_encode: (records uint32[n_tiles * UMI_TILE, UMI_REC_WORDS], tiles uint32[n_tiles, UMI_TILE_WORDS])."""
    text, off = text_and_offsets(umis)
    n = len(off) - 1
    t = _buf(text)
    n_tiles = check(lib().dcrx_umi_encode(t.ctypes.data, off.ctypes.data, n, None, None))
    recs = np.zeros((max(n_tiles, 1) * UMI_TILE, UMI_REC_WORDS), dtype=np.uint32)
    tiles = np.zeros((max(n_tiles, 1), UMI_TILE_WORDS), dtype=np.uint32)
    check(lib().dcrx_umi_encode(t.ctypes.data, off.ctypes.data, n, recs.ctypes.data, tiles.ctypes.data))
    return recs[:n_tiles * UMI_TILE], tiles[:n_tiles]


def umi_neighbours_keys(umis, k: int, cap: int | None = None) -> np.ndarray:
    """dcrx_umi_neighbours on the current device: uint64 keys (i << 32 | j), i < j, ascending.  `cap`: the first call's room
    (a call that finds more pairs is repeated with room for all of them)."""
    text, off = text_and_offsets(umis)
    n = len(off) - 1
    t = _buf(text)
    if k < 0:
        raise ValueError("the UMI distance threshold (-bc) must be >= 0")
    cap = int(4 * n + 1024) if cap is None else int(cap)
    for _ in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint64)
        total = check(lib().dcrx_umi_neighbours(t.ctypes.data, off.ctypes.data, n, int(k), out.ctypes.data, cap))
        if total <= cap:
            return out[:total]
        cap = total
    raise DcrxError(-1, "dcrx_umi_neighbours: the pair count changed between two calls")


def umi_neighbours(umis, k: int):
    """Every pair (i, j), i < j, of UMIs within Levenshtein distance k, ascending: (rows, cols) as int64 arrays.  The one
    function collapse.make_merge_groups calls for the search (tests on a CPU-only host put a stand-in here)."""
    keys = umi_neighbours_keys(umis, k)
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def seqs_equivalent(a: str, b: str, lev_fraction: float) -> bool:
    """dcrx_seqs_equivalent: the host's are_seqs_equivalent."""
    ab, bb = a.encode("latin-1"), b.encode("latin-1")
    return bool(check(lib().dcrx_seqs_equivalent(ab, len(ab), bb, len(bb), float(lev_fraction))))


class Groups:
    """dcrx_collapse_group's handle over the rows of a front half (keeps the text and rows it points into alive)."""

    def __init__(self, text: bytes, offsets, rows, field_sep: str, lev_fraction: float, sampling_analysis: bool):
        self._text = _buf(text)
        self._off = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._rows = np.ascontiguousarray(rows)
        h = C.c_void_p()
        cnt = np.zeros(len(GRP_COUNTERS), dtype=np.uint64)
        check(lib().dcrx_collapse_group(self._text.ctypes.data, len(text), self._off.ctypes.data, self._rows.ctypes.data, len(self._rows),
                                        field_sep.encode("ascii"), float(lev_fraction), int(bool(sampling_analysis)), C.byref(h),
                                        cnt.ctypes.data))
        self.handle = h.value
        self.counters = dict(zip(GRP_COUNTERS, (int(x) for x in cnt)))
        ng, nm, ub, pb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().dcrx_groups_info(self.handle, C.byref(ng), C.byref(nm), C.byref(ub), C.byref(pb)))
        self.n_groups = int(ng.value)
        umi, umi_off = np.zeros(max(ub.value, 1), dtype=np.uint8), np.zeros(self.n_groups + 1, dtype=np.uint64)
        proto, proto_off = np.zeros(max(pb.value, 1), dtype=np.uint8), np.zeros(self.n_groups + 1, dtype=np.uint64)
        self.member_off = np.zeros(self.n_groups + 1, dtype=np.uint64)
        self.member_rows = np.zeros(max(nm.value, 1), dtype=np.uint64)
        check(lib().dcrx_groups_export(self.handle, umi.ctypes.data, umi_off.ctypes.data, proto.ctypes.data, proto_off.ctypes.data,
                                       self.member_off.ctypes.data, self.member_rows.ctypes.data))
        self.member_rows = self.member_rows[:nm.value]
        self.umi_text, self.umi_off = umi.tobytes()[:ub.value], umi_off
        self.proto_text, self.proto_off = proto.tobytes()[:pb.value], proto_off

    def umi(self, g: int) -> str:
        return self.umi_text[int(self.umi_off[g]):int(self.umi_off[g + 1])].decode("latin-1")

    def protoseq(self, g: int) -> str:
        return self.proto_text[int(self.proto_off[g]):int(self.proto_off[g + 1])].decode("latin-1")

    def equivalent(self, rows, cols, lev_fraction: float, n_threads: int = 0) -> np.ndarray:
        """make_clusters' edge test on the pairs (rows[e], cols[e]): a bool per pair."""
        keys = (np.asarray(rows, dtype=np.uint64) << np.uint64(32)) | np.asarray(cols, dtype=np.uint64)
        keys = np.ascontiguousarray(keys)
        keep = np.zeros(max(len(keys), 1), dtype=np.uint8)
        check(lib().dcrx_groups_equivalent(self.handle, keys.ctypes.data, len(keys), float(lev_fraction), keep.ctypes.data, int(n_threads)))
        return keep[:len(keys)].astype(bool)

    def count(self, cluster_groups, cluster_off, extra: bool = False):
        """dcrx_collapse_count: (votes, size_sum, freq text, -wc text or None, -bd text or None)."""
        cg = np.ascontiguousarray(cluster_groups, dtype=np.uint32)
        co = np.ascontiguousarray(cluster_off, dtype=np.uint64)
        nc = len(co) - 1
        nd, fb, wb, bb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        L = lib()
        check(L.dcrx_collapse_count(self.handle, cg.ctypes.data, co.ctypes.data, nc, C.byref(nd), None, None, C.byref(fb), None,
                                    int(extra), C.byref(wb), None, C.byref(bb), None))
        votes = np.zeros(max(nd.value, 1), dtype=np.uint64)
        ssum = np.zeros(max(nd.value, 1), dtype=np.uint64)
        freq = np.zeros(max(fb.value, 1), dtype=np.uint8)
        wc = np.zeros(max(wb.value, 1), dtype=np.uint8)
        bd = np.zeros(max(bb.value, 1), dtype=np.uint8)
        check(L.dcrx_collapse_count(self.handle, cg.ctypes.data, co.ctypes.data, nc, C.byref(nd), votes.ctypes.data, ssum.ctypes.data,
                                    C.byref(fb), freq.ctypes.data, int(extra), C.byref(wb), wc.ctypes.data, C.byref(bb), bd.ctypes.data))
        n = int(nd.value)
        return (votes[:n], ssum[:n], freq.tobytes()[:fb.value], wc.tobytes()[:wb.value] if extra else None,
                bd.tobytes()[:bb.value] if extra else None)

    def close(self):
        if getattr(self, "handle", None):
            lib().dcrx_groups_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cdr3GenesC(C.Structure):
    _fields_ = [("n_v", C.c_uint32), ("n_j", C.c_uint32),
                ("v_regions", C.c_void_p), ("v_region_off", C.c_void_p), ("j_regions", C.c_void_p), ("j_region_off", C.c_void_p),
                ("v_pos", C.c_void_p), ("v_res", C.c_void_p), ("v_res_off", C.c_void_p),
                ("j_pos", C.c_void_p), ("j_motif", C.c_void_p), ("j_motif_off", C.c_void_p)]


CDR3_ROW_DTYPE = np.dtype([("seq_off", "<u8"), ("aa_off", "<u8"), ("seq_len", "<u4"), ("aa_len", "<u4"), ("junction_off", "<u4"),
                           ("junction_len", "<u4"), ("junction_aa_off", "<u4"), ("junction_aa_len", "<u4"), ("start_cdr3", "<i4"),
                           ("end_cdr3", "<i4"), ("bad_codon_at", "<u4"), ("status", "u1"), ("productive", "u1"), ("in_frame", "u1"),
                           ("stop", "u1"), ("conserved_c", "u1"), ("conserved_f", "u1"), ("pad", "u1", (2,)), ("reserved", "<u4")])
CDR3_OK, CDR3_INDEX_ERROR, CDR3_BAD_CODON, CDR3_MOTIF_LEFT = 0, 1, 2, 3


class Cdr3Genes:
    """The gene tables of dcrx_cdr3_batch (the reference's import_gene_information, translate.py:163-254) as texts and offsets."""

    def __init__(self, v_regions, j_regions, v_pos, v_res, j_pos, j_motif):
        def blob(strings, off_dtype):
            bs = [str(x).encode("latin-1") for x in strings]
            off = np.zeros(len(bs) + 1, dtype=off_dtype)
            off[1:] = np.cumsum([len(b) for b in bs])
            return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy(), off
        self.n_v, self.n_j = len(v_regions), len(j_regions)
        self._keep = [blob(v_regions, np.uint64), blob(j_regions, np.uint64), blob(v_res, np.uint32), blob(j_motif, np.uint32),
                      np.ascontiguousarray(v_pos, dtype=np.int32), np.ascontiguousarray(j_pos, dtype=np.int32)]
        (vr, vo), (jr, jo), (vs, vso), (jm, jmo), vp_, jp_ = self._keep
        self.c = Cdr3GenesC(self.n_v, self.n_j, vr.ctypes.data, vo.ctypes.data, jr.ctypes.data, jo.ctypes.data,
                            vp_.ctypes.data, vs.ctypes.data, vso.ctypes.data, jp_.ctypes.data, jm.ctypes.data, jmo.ctypes.data)


def cdr3_batch(genes: Cdr3Genes, v, j, vdel, jdel, inserts):
    """dcrx_cdr3_batch: (rows[CDR3_ROW_DTYPE], text bytes) for the DCRs (v, j, vdel, jdel: integers; inserts: strings)."""
    n = len(v)
    v, j, vdel, jdel = (np.ascontiguousarray(x, dtype=np.int32) for x in (v, j, vdel, jdel))
    ib = [str(x).encode("latin-1") for x in inserts]
    ioff = np.zeros(n + 1, dtype=np.uint64)
    ioff[1:] = np.cumsum([len(b) for b in ib])
    itext = np.frombuffer(b"".join(ib) + b"\0", dtype=np.uint8).copy()
    rows = np.zeros(n, dtype=CDR3_ROW_DTYPE)
    assert CDR3_ROW_DTYPE.itemsize == 64
    args = (C.byref(genes.c), n, v.ctypes.data, j.ctypes.data, vdel.ctypes.data, jdel.ctypes.data, itext.ctypes.data, ioff.ctypes.data, rows.ctypes.data)
    need = int(lib().dcrx_cdr3_batch(*args, None, 0))
    if need < 0:
        check(need)
    text = np.zeros(max(need, 1), dtype=np.uint8)
    got = int(lib().dcrx_cdr3_batch(*args, text.ctypes.data, need))
    if got < 0:
        check(got)
    return rows, text.tobytes()


class TuneStateC(C.Structure):
    _fields_ = [("rescue_waves", C.c_uint32), ("launches", C.c_uint32), ("us_first", C.c_float), ("us_second", C.c_float),
                ("launch_form", C.c_uint32), ("candidates", C.c_uint32)]


class SynthCfgC(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("read_len", C.c_uint32), ("p_rearranged", C.c_float),
                ("sub_rate", C.c_float), ("n_rate", C.c_float)]


MERGE_ANCHOR = 32            # DCRX_MERGE_ANCHOR
MERGE_MAX_JUNCTION = 128     # DCRX_MERGE_MAX_JUNCTION
MERGE_STATS = ("entries_in", "roots_out", "out_of_reach", "merged", "reads_moved", "longest_chain")


class MergeStatsC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in MERGE_STATS]


CLONOTYPE_STATS = ("entries_in", "reads_in", "productive", "productive_reads", "nonproductive", "nonproductive_reads",
                   "untranslatable", "untranslatable_reads", "clonotypes_out", "convergent", "largest_n_dcrs")
CLONOTYPE_COLUMNS = ["v_call", "j_call", "junction_aa", "duplicate_count", "n_dcrs", "junction", "decombinator_id", "top_dcr_count"]
NOT_A_MEMBER = 0xFFFFFFFF      # clonotype_of of an entry that is in no clonotype
CLONO_MAX_ENTRIES = 1 << 30    # dcrx_clonotypes / dcrx_cdr3_device: DCRX_E_UNSUPPORTED from here on
E_UNSUPPORTED = -2             # DCRX_E_UNSUPPORTED


class ClonotypeStatsC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in CLONOTYPE_STATS]


CDR3_NETWORK_STATS = ("nodes_in", "out_of_reach", "edges", "clusters_out", "singletons", "largest_cluster", "largest_degree")
CDR3_CLUSTER_COLUMNS = ["clonotype", "v_call", "j_call", "junction_aa", "duplicate_count", "cluster", "cluster_size",
                        "cluster_duplicate_count", "degree"]
CDR3_EDGE_COLUMNS = ["a", "b", "distance"]
CDR3NET_MAX_LEN = 32           # DCRX_CDR3NET_MAX_LEN
CDR3NET_MAX_NODES = 1 << 30    # dcrx_cdr3_network / dcrx_cdr3_neighbours_device: DCRX_E_UNSUPPORTED from here on
CDR3_METRICS = {"hamming": 0, "levenshtein": 1}      # DCRX_CDR3NET_HAMMING, DCRX_CDR3NET_LEVENSHTEIN


class Cdr3NetworkStatsC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in CDR3_NETWORK_STATS]


CDR3_MATCH_STATS = ("queries", "targets", "queries_out_of_reach", "targets_out_of_reach", "hits", "queries_hit", "queries_hit_weight",
                    "targets_hit", "largest_degree")
CDR3_MATCH_MAX_SAMPLES = 64         # files of one `match` call
CDR3_MATCH_COLUMNS = ["clonotype", "v_call", "j_call", "junction_aa", "duplicate_count", "target", "distance"]      # then db_<column> ...
CDR3_METRIC_WEIGHTED = 2            # DCRX_CDR3NET_WEIGHTED: the weighted entries' own (the *_metric entries refuse it)
CDR3_COST_MAX_GAP, CDR3_COST_MAX_TRIM, CDR3_MAX_RADIUS = 255, 16, 65535
AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"
# The default substitution costs, after TCRdist: 3 * min(4, 4 - BLOSUM62) off the diagonal, which is 12 for every pair of
# letters but the pairs BLOSUM62 scores above zero, spelt out here by score (B, J, O, U, X and Z cost 12 against everything).
CDR3_COST_FAR = 12
CDR3_COST_NEAR = {
    9: ("AS", "RQ", "ND", "NH", "NS", "QK", "EK", "IM", "LV", "MV", "FW", "ST"),      # BLOSUM62 score 1
    6: ("RK", "DE", "QE", "HY", "IL", "LM", "WY"),                                    # score 2
    3: ("IV", "FY"),                                                                  # score 3
}


class Cdr3MatchStatsC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in CDR3_MATCH_STATS]


class Cdr3CostC(C.Structure):      # dcrx_cdr3_cost_t
    _fields_ = [("sub", (C.c_uint8 * 32) * 32), ("gap", C.c_uint32), ("ntrim", C.c_uint32), ("ctrim", C.c_uint32)]


CDR3_PROFILE_MAX_BINS = 32           # dcrx_cdr3_profile_weighted: bins 1 .. 32, step 1 .. 65535, step * (bins - 1) <= 65535
CDR3_PROFILE_STATS = ("queries", "targets", "queries_out_of_reach", "queries_not_letters", "targets_out_of_reach", "cells_sum",
                      "queries_nonzero")


class Cdr3ProfileStatsC(C.Structure):      # dcrx_cdr3_profile_stats_t
    _fields_ = [(k, C.c_uint64) for k in CDR3_PROFILE_STATS]


CDR3_NO_RADIUS = 0xFFFFFFFF          # DCRX_CDR3_NO_RADIUS: a target of dcrx_cdr3_tally_weighted that takes part in nothing
CDR3_TALLY_MAX_SAMPLES = 64          # files of one `tabulate` call
CDR3_TALLY_STATS = ("queries", "targets", "queries_out_of_reach", "queries_not_letters", "targets_out_of_reach",
                    "targets_without_radius", "hits", "queries_hit", "queries_hit_weight", "targets_hit")


class Cdr3TallyStatsC(C.Structure):      # dcrx_cdr3_tally_stats_t
    _fields_ = [(k, C.c_uint64) for k in CDR3_TALLY_STATS]


CDR3_MOTIF_MAX_SAMPLES = 64          # files of one `motifs` call
CDR3_MOTIF_MAX_TRIM = 16             # DCRX_CDR3_MOTIF_MAX_TRIM
CDR3_MOTIF_MAX_RESAMPLES = 65535     # DCRX_CDR3_MOTIF_MAX_RESAMPLES
CDR3_MOTIF_KS = (2, 3, 4)            # DCRX_CDR3_MOTIF_K_ALL: a k_mask has bit k set for every k of K
CDR3_MOTIF_MAX_UNITS = 1 << 30       # dcrx_cdr3_motifs: DCRX_E_UNSUPPORTED from here on
CDR3_MOTIF_STATS = ("sample_units", "sample_take_part", "sample_out_of_reach", "sample_not_letters", "background_units",
                    "background_take_part", "background_out_of_reach", "background_not_letters", "motifs", "reported")
CDR3_MOTIF_OUTPUTS = (("k", np.uint32), ("code", np.uint32), ("cs", np.uint32), ("cb", np.uint32), ("ge", np.uint32), ("sum", np.uint64),
                      ("max", np.uint32))
CDR3_MOTIF_COLUMNS = ["motif", "k", "cdr3s", "background_cdr3s", "resamples", "resamples_at_least", "resample_sum", "resample_max",
                      "expected", "fold", "p_value"]


class Cdr3MotifStatsC(C.Structure):      # dcrx_cdr3_motif_stats_t
    _fields_ = [(k, C.c_uint64) for k in CDR3_MOTIF_STATS]


CDR3_MOTIF_COUNT = 26 ** 2 + 26 ** 3 + 26 ** 4      # 475 228: every motif, and the most that can be selected
CDR3_MOTIF_GROUP_STATS = ("units", "take_part", "selected", "member_pairs", "global_edges", "groups", "singleton_groups", "largest_group",
                          "mixed_groups", "rounds")
CDR3_GROUP_COLUMNS = ["junction_aa", "clonotypes", "duplicate_count", "group", "group_cdr3s", "group_duplicate_count", "degree", "motifs"]
CDR3_MOTIF_MEMBER_COLUMNS = ["motif", "k", "junction_aa", "position", "group"]


class Cdr3MotifGroupStatsC(C.Structure):      # dcrx_cdr3_motif_group_stats_t
    _fields_ = [(k, C.c_uint64) for k in CDR3_MOTIF_GROUP_STATS]


OVERLAP_MAX_SAMPLES = 64       # DCRX_OVERLAP_MAX_SAMPLES
OVERLAP_MAX_ROWS = 1 << 30     # dcrx_overlap_run: DCRX_E_UNSUPPORTED from here on
OVERLAP_PLANES = ("shared", "shared_weight", "min_weight", "prod_lo", "prod_hi")      # enum dcrx_overlap_plane
OVERLAP_STATS = ("rows_in", "groups", "private_groups", "shared_groups", "in_all_samples", "largest_n_samples", "public_rows",
                 "public_cells")
OVERLAP_PUBLIC_COLUMNS = ["v_call", "j_call", "junction_aa", "n_samples", "duplicate_count"]      # then one column per sample
OVERLAP_PAIR_COLUMNS = ["sample_a", "sample_b", "clonotypes_a", "clonotypes_b", "shared_clonotypes", "reads_a", "reads_b",
                        "shared_reads_a", "shared_reads_b", "min_reads", "jaccard", "overlap_coefficient", "bray_curtis",
                        "morisita_horn"]


class OverlapStatsC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in OVERLAP_STATS]


ASSOC_MAX_SAMPLES = 64                  # DCRX_ASSOC_MAX_SAMPLES: a presence pattern and a relabeling are one uint64
ASSOC_WIDE_MAX_SAMPLES = 1024           # DCRX_ASSOC_WIDE_MAX_SAMPLES: patterns and relabelings of up to 16 words
ASSOC_MAX_PERMUTATIONS = 1 << 20        # DCRX_ASSOC_MAX_PERMUTATIONS
ASSOC_MAX_FEATURES = 1 << 30            # dcrx_assoc_permute: DCRX_E_UNSUPPORTED from here on
ASSOC_STATS = ("features", "features_weighted", "weight", "permutations", "tail_total", "min_perm_rank")
ASSOC_OUTPUTS = ("obs_rank", "labels", "perm_min", "tail")
ASSOC_RANKSUM_PLANES = 7                # DCRX_ASSOC_RANKSUM_PLANES: a score is 0 .. 2 N - 2 <= 126
ASSOC_RANKSUM_SHIFT = 20                # DCRX_ASSOC_RANKSUM_SHIFT: t = (u scale) >> 20, u clamped to 20 bits
ASSOC_RANKSUM_MAX_EDGES = 1024          # DCRX_ASSOC_RANKSUM_MAX_EDGES
ASSOC_RANKSUM_ALTERNATIVES = ("greater", "less", "two-sided")      # the alternative, by number
ASSOC_RANKSUM_STATS = ("features", "features_weighted", "weight", "permutations", "tail_total", "max_perm_score")
ASSOC_RANKSUM_OUTPUTS = ("obs_score", "labels", "perm_max", "exceed", "tail")


class AssocStatsC(C.Structure):      # dcrx_assoc_stats_t
    _fields_ = [(k, C.c_uint64) for k in ASSOC_STATS]


class AssocRanksumStatsC(C.Structure):      # dcrx_assoc_ranksum_stats_t
    _fields_ = [(k, C.c_uint64) for k in ASSOC_RANKSUM_STATS]


DOWNSAMPLE_MAX_SAMPLES = 4096      # DCRX_DOWNSAMPLE_MAX_SAMPLES
DOWNSAMPLE_MAX_ROWS = 1 << 30      # dcrx_downsample: DCRX_E_UNSUPPORTED from here on
DOWNSAMPLE_MAX_READS = 1 << 40     # ... and for this many reads in all
DOWNSAMPLE_OUTPUTS = ("kept", "reads", "depth_used", "threshold")
OVERLAP_DIVERSITY_COLUMNS = ["sample", "reads_in", "reads", "clonotypes", "singletons", "doubletons", "max_reads", "d50", "chao1",
                             "simpson", "inverse_simpson", "gini", "shannon", "clonality"]


# dcrx_clono_row_t: what dcrx_cdr3_device leaves of an entry (flags: productive, in_frame, stop, conserved_c, conserved_f from bit 0)
CLONO_ROW_DTYPE = np.dtype([("hash", "<u8"), ("arena_off", "<u8"), ("start_cdr3", "<i4"), ("end_cdr3", "<i4"), ("seq_len", "<u4"),
                            ("status", "u1"), ("flags", "u1"), ("pad", "<u2")])


# every symbol include/dcrx.h and include/dcrx_synth.h declare
EXPORTS = [
    "dcrx_umi_encode", "dcrx_umi_neighbours_device", "dcrx_umi_neighbours", "dcrx_collapse_group",
    "dcrx_groups_destroy", "dcrx_groups_info", "dcrx_groups_export", "dcrx_groups_equivalent", "dcrx_collapse_count",
    "dcrx_seqs_equivalent",
    "dcrx_tables_create", "dcrx_tables_destroy", "dcrx_tables_info", "dcrx_pack_reads", "dcrx_pack_reads_span",
    "dcrx_unpack_reads", "dcrx_fastq_open", "dcrx_fastq_open_range", "dcrx_fastq_lines", "dcrx_fastq_close", "dcrx_fastq_next", "dcrx_count_prefix_byte", "dcrx_assemble_rows",
    "dcrx_decombine", "dcrx_decombine_chains", "dcrx_decombine_device", "dcrx_set_timing_events", "dcrx_set_step_events", "dcrx_reserve_device", "dcrx_compact_hits_device",
    "dcrx_compact_hits_bitmap_device", "dcrx_compact_hits_packed_device", "dcrx_set_reserved_cus", "dcrx_tune_state", "dcrx_cdr3_batch",
    "dcrx_device_count", "dcrx_set_device", "dcrx_device_name", "dcrx_malloc_device", "dcrx_free_device",
    "dcrx_malloc_host", "dcrx_free_host", "dcrx_memcpy_h2d", "dcrx_memcpy_d2h", "dcrx_memset_device", "dcrx_synchronize", "dcrx_event_create",
    "dcrx_event_destroy", "dcrx_event_record", "dcrx_event_elapsed_ms", "dcrx_abi_version", "dcrx_last_error",
    "dcrx_compact_hits_packed8_device", "dcrx_tuple_layout", "dcrx_tuple_message_bytes", "dcrx_compact_hits_narrow_device", "dcrx_set_tuple_sink", "dcrx_collapse_front", "dcrx_spacer_search", "dcrx_gzip_open", "dcrx_gzip_write", "dcrx_gzip_close", "dcrx_build_info", "dcrx_synth_reads_host", "dcrx_synth_reads_device", "dcrx_synth_exceptions_host",
    "dcrx_set_tune_wait", "dcrx_comm_available", "dcrx_comm_unique_id", "dcrx_comm_create", "dcrx_comm_create_all", "dcrx_comm_destroy", "dcrx_comm_info",
    "dcrx_comm_allreduce_u64", "dcrx_comm_allreduce_f64", "dcrx_comm_allgather", "dcrx_comm_gather_v", "dcrx_comm_barrier", "dcrx_comm_allgather_host",
    "dcrx_comm_allreduce_host_u64", "dcrx_decombine_sharded", "dcrx_event_synchronize", "dcrx_event_create_ordering", "dcrx_stream_create", "dcrx_stream_destroy", "dcrx_stream_synchronize",
    "dcrx_stream_wait_event", "dcrx_memcpy_d2h_async", "dcrx_memcpy_d2d_async", "dcrx_memset_device_async",
    "dcrx_counts_create", "dcrx_counts_destroy", "dcrx_counts_reset", "dcrx_counts_set_hash_bits", "dcrx_count_device", "dcrx_decombine_count",
    "dcrx_decombine_chains_count", "dcrx_counts_read", "dcrx_format_counts",
    "dcrx_merge_work_bytes", "dcrx_merge_parents_device", "dcrx_merge_dcrs", "dcrx_merge_gather",
    "dcrx_clono_genes_create", "dcrx_clono_genes_destroy", "dcrx_clono_set_hash_bits", "dcrx_clono_work_bytes", "dcrx_cdr3_device",
    "dcrx_clonotypes", "dcrx_clonotypes_text", "dcrx_format_clonotypes",
    "dcrx_cdr3net_work_bytes", "dcrx_cdr3_neighbours_device", "dcrx_cdr3_network", "dcrx_format_cdr3_clusters",
    "dcrx_format_cdr3_edges",
    "dcrx_cdr3net_metric_work_bytes", "dcrx_cdr3_neighbours_metric_device", "dcrx_cdr3_network_metric", "dcrx_format_cdr3_edges_metric",
    "dcrx_overlap_set_hash_bits", "dcrx_overlap_run", "dcrx_overlap_destroy", "dcrx_overlap_info", "dcrx_overlap_export",
    "dcrx_overlap_pairs_device", "dcrx_format_overlap_public",
    "dcrx_downsample_work_bytes", "dcrx_downsample_device", "dcrx_downsample", "dcrx_abundance_classes",
    "dcrx_cdr3_index_create", "dcrx_cdr3_index_destroy", "dcrx_cdr3_index_info", "dcrx_cdr3_match_work_bytes", "dcrx_cdr3_match_device",
    "dcrx_cdr3_match_run", "dcrx_cdr3_match_destroy", "dcrx_cdr3_match_info", "dcrx_cdr3_match_export", "dcrx_format_cdr3_matches",
    "dcrx_cdr3_match_weighted_work_bytes", "dcrx_cdr3_match_weighted_device", "dcrx_cdr3_match_weighted_run", "dcrx_cdr3_match_export_dist",
    "dcrx_format_cdr3_matches_weighted",
    "dcrx_cdr3net_weighted_work_bytes", "dcrx_cdr3_neighbours_weighted_device", "dcrx_cdr3_network_weighted",
    "dcrx_format_cdr3_edges_weighted",
    "dcrx_cdr3_motifs_work_bytes", "dcrx_cdr3_motifs_device", "dcrx_cdr3_motifs",
    "dcrx_cdr3_motif_members_work_bytes", "dcrx_cdr3_motif_members_device", "dcrx_cdr3_groups_work_bytes", "dcrx_cdr3_groups_device",
    "dcrx_cdr3_motif_groups",
    "dcrx_cdr3_profile_weighted_work_bytes", "dcrx_cdr3_profile_weighted_device", "dcrx_cdr3_profile_weighted",
    "dcrx_cdr3_tally_weighted_work_bytes", "dcrx_cdr3_tally_weighted_device", "dcrx_cdr3_tally_weighted",
    "dcrx_assoc_permute_device", "dcrx_assoc_permute",
    "dcrx_assoc_permute_wide_device", "dcrx_assoc_permute_wide",
    "dcrx_assoc_ranksum_device", "dcrx_assoc_ranksum",
]

_lib = None


def lib():
    """The loaded library; raises ImportError with build instructions when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback for the decombine hot path.")
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    sig = {
        "dcrx_tables_create": (i32, [C.POINTER(TagSetC), C.POINTER(vp)]),
        "dcrx_tables_destroy": (None, [vp]),
        "dcrx_tables_info": (i32, [vp, C.POINTER(TablesInfoC)]),
        "dcrx_pack_reads": (C.c_int64, [vp, vp, u64, u32, vp, vp, vp, vp, vp, u64]),
        "dcrx_pack_reads_span": (C.c_int64, [vp, vp, vp, u64, u32, vp, vp, vp, vp, vp, u64]),
        "dcrx_unpack_reads": (i32, [C.POINTER(BatchC), vp, vp]),
        "dcrx_fastq_open": (i32, [C.c_char_p, i32, C.POINTER(vp)]),
        "dcrx_fastq_close": (None, [vp]),
        "dcrx_fastq_open_range": (i32, [C.c_char_p, u64, u64, C.POINTER(vp)]),
        "dcrx_fastq_lines": (i32, [C.c_char_p, u64, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]),
        "dcrx_fastq_next": (i32, [vp, u64, C.POINTER(FastqBatchC)]),
        "dcrx_count_prefix_byte": (u64, [vp, vp, vp, u64, u32, i32]),
        "dcrx_assemble_rows": (C.c_int64, [vp, u64, C.POINTER(SpansC), C.POINTER(SpansC), C.POINTER(SpansC),
                                           C.POINTER(SpansC), C.POINTER(SpansC), C.POINTER(SpansC), C.c_char_p, vp, u64,
                                           C.POINTER(u64)]),
        "dcrx_decombine": (i32, [vp, C.POINTER(CfgC), C.POINTER(BatchC), vp, vp]),
        "dcrx_decombine_chains": (i32, [vp, u32, C.POINTER(CfgC), C.POINTER(BatchC), vp, vp]),
        "dcrx_decombine_device": (i32, [vp, C.POINTER(CfgC), C.POINTER(BatchC), vp, vp, vp]),
        "dcrx_set_timing_events": (i32, [vp, vp, vp]),
        "dcrx_set_step_events": (i32, [vp, vp, vp]),
        "dcrx_reserve_device": (i32, [vp, u64]),
        "dcrx_compact_hits_device": (i32, [vp, u64, u64, vp, vp, vp, vp]),
        "dcrx_compact_hits_bitmap_device": (i32, [vp, u64, vp, vp, vp, vp]),
        "dcrx_compact_hits_packed_device": (i32, [vp, u64, vp, vp, vp, vp]),
        "dcrx_compact_hits_packed8_device": (i32, [vp, u64, vp, vp, vp, vp]),
        "dcrx_tuple_layout": (i32, [vp, u32, C.POINTER(TupleLayoutC)]),
        "dcrx_tuple_message_bytes": (u64, [C.POINTER(TupleLayoutC), u64, u64]),
        "dcrx_compact_hits_narrow_device": (i32, [vp, C.POINTER(TupleLayoutC), vp, u64, u64, vp, vp, vp]),
        "dcrx_set_tuple_sink": (i32, [vp, C.POINTER(TupleLayoutC), vp, u64, vp]),
        "dcrx_collapse_front": (C.c_int64, [vp, u64, C.POINTER(CollapseCfgC), vp, u64, vp, vp, i32]),
        "dcrx_spacer_search": (i32, [C.c_char_p, i32, C.c_char_p, i32, vp, vp, i32, C.POINTER(C.c_int32)]),
        "dcrx_umi_encode": (C.c_int64, [vp, vp, u64, vp, vp]),
        "dcrx_umi_neighbours_device": (i32, [vp, vp, u64, C.c_int32, vp, u64, vp, vp]),
        "dcrx_umi_neighbours": (C.c_int64, [vp, vp, u64, C.c_int32, vp, u64]),
        "dcrx_collapse_group": (i32, [vp, u64, vp, vp, u64, C.c_char_p, C.c_double, i32, C.POINTER(vp), vp]),
        "dcrx_groups_destroy": (None, [vp]),
        "dcrx_groups_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "dcrx_groups_export": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "dcrx_groups_equivalent": (i32, [vp, vp, u64, C.c_double, vp, i32]),
        "dcrx_collapse_count": (i32, [vp, vp, vp, u64, C.POINTER(u64), vp, vp, C.POINTER(u64), vp, i32, C.POINTER(u64), vp,
                                      C.POINTER(u64), vp]),
        "dcrx_seqs_equivalent": (i32, [C.c_char_p, u32, C.c_char_p, u32, C.c_double]),
        "dcrx_set_reserved_cus": (i32, [vp, u32]),
        "dcrx_tune_state": (i32, [vp, i32, u64, C.POINTER(TuneStateC)]),
        "dcrx_cdr3_batch": (C.c_int64, [C.POINTER(Cdr3GenesC), u64, vp, vp, vp, vp, vp, vp, vp, vp, u64]),
        "dcrx_gzip_open": (i32, [C.c_char_p, i32, i32, C.POINTER(vp)]),
        "dcrx_gzip_write": (i32, [vp, vp, u64]),
        "dcrx_gzip_close": (i32, [vp]),
        "dcrx_device_count": (i32, []),
        "dcrx_set_device": (i32, [i32]),
        "dcrx_device_name": (i32, [C.c_char_p, C.c_size_t]),
        "dcrx_malloc_device": (i32, [C.POINTER(vp), C.c_size_t]),
        "dcrx_free_device": (i32, [vp]),
        "dcrx_malloc_host": (i32, [C.POINTER(vp), C.c_size_t]),
        "dcrx_free_host": (i32, [vp]),
        "dcrx_memcpy_h2d": (i32, [vp, vp, C.c_size_t]),
        "dcrx_memcpy_d2h": (i32, [vp, vp, C.c_size_t]),
        "dcrx_memset_device": (i32, [vp, i32, C.c_size_t]),
        "dcrx_synchronize": (i32, []),
        "dcrx_event_create": (i32, [C.POINTER(vp)]),
        "dcrx_event_destroy": (i32, [vp]),
        "dcrx_event_record": (i32, [vp, vp]),
        "dcrx_event_elapsed_ms": (i32, [vp, vp, C.POINTER(C.c_float)]),
        "dcrx_abi_version": (i32, []),
        "dcrx_last_error": (C.c_char_p, []),
        "dcrx_build_info": (C.c_char_p, []),
        "dcrx_synth_reads_host": (i32, [vp, C.POINTER(SynthCfgC), u64, u64, u32, vp]),
        "dcrx_synth_reads_device": (i32, [vp, C.POINTER(SynthCfgC), u64, u64, u32, vp, vp]),
        "dcrx_synth_exceptions_host": (C.c_int64, [vp, C.POINTER(SynthCfgC), u64, u64, vp, vp, vp, u64]),
        "dcrx_set_tune_wait": (i32, [vp, i32]),
        "dcrx_comm_available": (i32, []),
        "dcrx_comm_unique_id": (i32, [vp]),
        "dcrx_comm_create": (i32, [vp, i32, i32, C.POINTER(vp)]),
        "dcrx_comm_create_all": (i32, [i32, vp, C.POINTER(vp)]),
        "dcrx_comm_destroy": (None, [vp]),
        "dcrx_comm_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "dcrx_comm_allreduce_u64": (i32, [vp, vp, vp, u64, i32, vp]),
        "dcrx_comm_allreduce_f64": (i32, [vp, vp, vp, u64, i32, vp]),
        "dcrx_comm_allgather": (i32, [vp, vp, vp, u64, vp]),
        "dcrx_comm_gather_v": (i32, [vp, vp, u64, vp, vp, i32, vp]),
        "dcrx_comm_barrier": (i32, [vp, vp]),
        "dcrx_comm_allgather_host": (i32, [vp, vp, vp, u64]),
        "dcrx_comm_allreduce_host_u64": (i32, [vp, vp, u64, i32]),
        "dcrx_decombine_sharded": (i32, [vp, vp, C.POINTER(CfgC), C.POINTER(BatchC), vp, vp, C.POINTER(TupleLayoutC), vp, u64, vp, vp, vp]),
        "dcrx_event_synchronize": (i32, [vp]),
        "dcrx_event_create_ordering": (i32, [C.POINTER(vp)]),
        "dcrx_stream_create": (i32, [C.POINTER(vp)]),
        "dcrx_stream_destroy": (i32, [vp]),
        "dcrx_stream_synchronize": (i32, [vp]),
        "dcrx_stream_wait_event": (i32, [vp, vp]),
        "dcrx_memcpy_d2h_async": (i32, [vp, vp, C.c_size_t, vp]),
        "dcrx_memcpy_d2d_async": (i32, [vp, vp, C.c_size_t, vp]),
        "dcrx_memset_device_async": (i32, [vp, i32, C.c_size_t, vp]),
        "dcrx_counts_create": (i32, [C.POINTER(vp)]),
        "dcrx_counts_destroy": (None, [vp]),
        "dcrx_counts_reset": (i32, [vp]),
        "dcrx_counts_set_hash_bits": (i32, [vp, u32]),
        "dcrx_count_device": (i32, [vp, vp, C.POINTER(BatchC), u64, vp, vp]),
        "dcrx_decombine_count": (i32, [vp, C.POINTER(CfgC), C.POINTER(BatchC), vp, u64, vp, vp]),
        "dcrx_decombine_chains_count": (i32, [vp, u32, C.POINTER(CfgC), C.POINTER(BatchC), vp, u64, vp, vp]),
        "dcrx_counts_read": (C.c_int64, [vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64, C.POINTER(u64)]),
        "dcrx_format_counts": (C.c_int64, [u64, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, vp, u64]),
        "dcrx_merge_gather": (C.c_int64, [u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dcrx_merge_work_bytes": (u64, [u64]),
        "dcrx_merge_parents_device": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, u32, u64, vp, vp, vp, u64, vp]),
        "dcrx_merge_dcrs": (C.c_int64, [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, C.POINTER(MergeStatsC)]),
        "dcrx_clono_genes_create": (i32, [C.POINTER(Cdr3GenesC), vp, vp, C.POINTER(vp)]),
        "dcrx_clono_genes_destroy": (None, [vp]),
        "dcrx_clono_set_hash_bits": (i32, [vp, u32]),
        "dcrx_clono_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_device": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_clonotypes": (C.c_int64, [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(ClonotypeStatsC)]),
        "dcrx_clonotypes_text": (C.c_int64, [vp, vp, u64]),
        "dcrx_format_clonotypes": (C.c_int64, [u64, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, u64]),
        "dcrx_cdr3net_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_neighbours_device": (i32, [u64, vp, vp, vp, u64, u32, vp, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_cdr3_network": (C.c_int64, [u64, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, u64, vp, C.POINTER(Cdr3NetworkStatsC)]),
        "dcrx_format_cdr3_clusters": (C.c_int64, [u64, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64]),
        "dcrx_format_cdr3_edges": (C.c_int64, [u64, vp, vp, vp, vp, vp, u64]),
        "dcrx_cdr3net_metric_work_bytes": (u64, [u64, u64, u32]),
        "dcrx_cdr3_neighbours_metric_device": (i32, [u64, vp, vp, vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_cdr3_network_metric": (C.c_int64, [u64, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                                 C.POINTER(Cdr3NetworkStatsC)]),
        "dcrx_format_cdr3_edges_metric": (C.c_int64, [u64, vp, vp, vp, vp, u32, vp, u64]),
        "dcrx_overlap_set_hash_bits": (i32, [u32]),
        "dcrx_overlap_run": (vp, [u32, u64, vp, vp, vp, vp, vp, u32, C.POINTER(i32)]),
        "dcrx_overlap_destroy": (None, [vp]),
        "dcrx_overlap_info": (i32, [vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(OverlapStatsC)]),
        "dcrx_overlap_export": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dcrx_overlap_pairs_device": (i32, [u64, vp, vp, vp, u32, vp, vp]),
        "dcrx_downsample_work_bytes": (u64, [u64, u32]),
        "dcrx_downsample_device": (i32, [u32, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp]),
        "dcrx_downsample": (i32, [u32, u64, vp, vp, vp, u64, vp, vp, vp, vp]),
        "dcrx_abundance_classes": (C.c_int64, [u32, u64, vp, vp, vp, vp, vp, vp]),
        "dcrx_format_overlap_public": (C.c_int64, [u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, u64, vp, vp, u32, vp, vp, u32, vp, vp, vp,
                                                   vp, vp, u64]),
        "dcrx_cdr3_index_create": (i32, [u64, vp, vp, vp, C.POINTER(vp)]),
        "dcrx_cdr3_index_destroy": (None, [vp]),
        "dcrx_cdr3_index_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "dcrx_cdr3_match_work_bytes": (u64, [u64, u64, u32]),
        "dcrx_cdr3_match_device": (i32, [vp, u64, vp, vp, vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_cdr3_match_run": (i32, [vp, u64, vp, vp, vp, vp, u32, u32, C.POINTER(vp)]),
        "dcrx_cdr3_match_destroy": (None, [vp]),
        "dcrx_cdr3_match_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(Cdr3MatchStatsC)]),
        "dcrx_cdr3_match_export": (i32, [vp, vp, vp, vp, vp, vp]),
        "dcrx_format_cdr3_matches": (C.c_int64, [u64, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp,
                                                 u32, vp, u64]),
        "dcrx_cdr3_match_weighted_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_match_weighted_device": (i32, [vp, u64, vp, vp, vp, u64, vp, u32, vp, vp, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_cdr3_match_weighted_run": (i32, [vp, u64, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
        "dcrx_cdr3_match_export_dist": (i32, [vp, vp]),
        "dcrx_format_cdr3_matches_weighted": (C.c_int64, [u64, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp,
                                                          vp, vp, vp, u64]),
        "dcrx_cdr3net_weighted_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_neighbours_weighted_device": (i32, [u64, vp, vp, vp, u64, vp, u32, vp, vp, vp, vp, u64, vp, vp, u64, vp]),
        "dcrx_cdr3_network_weighted": (C.c_int64, [u64, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                                   C.POINTER(Cdr3NetworkStatsC)]),
        "dcrx_format_cdr3_edges_weighted": (C.c_int64, [u64, vp, vp, vp, vp, vp, vp, u64]),
        "dcrx_cdr3_motifs_work_bytes": (u64, [u64, u64, u32]),
        "dcrx_cdr3_motifs_device": (i32, [u64, vp, vp, u64, vp, vp, u32, u32, u32, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, u64, vp]),
        "dcrx_cdr3_motifs": (i32, [u64, vp, vp, u64, vp, vp, u32, u32, u32, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp,
                                   C.POINTER(Cdr3MotifStatsC)]),
        "dcrx_cdr3_motif_members_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_motif_members_device": (i32, [u64, vp, vp, u32, u32, u32, u64, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp]),
        "dcrx_cdr3_groups_work_bytes": (u64, [u64, u64]),
        "dcrx_cdr3_groups_device": (i32, [u64, vp, vp, vp, u64, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp]),
        "dcrx_cdr3_motif_groups": (i32, [u64, vp, vp, vp, u32, u32, u32, u64, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                         C.POINTER(Cdr3MotifGroupStatsC)]),
        "dcrx_cdr3_profile_weighted_work_bytes": (u64, [u64, u64, u32]),
        "dcrx_cdr3_profile_weighted_device": (i32, [vp, u64, vp, vp, vp, u64, vp, u32, u32, vp, vp, u64, vp]),
        "dcrx_cdr3_profile_weighted": (i32, [vp, u64, vp, vp, vp, vp, u32, u32, vp, C.POINTER(Cdr3ProfileStatsC)]),
        "dcrx_cdr3_tally_weighted_work_bytes": (u64, [u64, u64, u64]),
        "dcrx_cdr3_tally_weighted_device": (i32, [vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp]),
        "dcrx_cdr3_tally_weighted": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Cdr3TallyStatsC)]),
        "dcrx_assoc_permute_device": (i32, [u32, u64, u64, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, vp]),
        "dcrx_assoc_permute": (i32, [u32, u64, u64, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, C.POINTER(AssocStatsC)]),
        "dcrx_assoc_permute_wide_device": (i32, [u32, vp, u64, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, vp]),
        "dcrx_assoc_permute_wide": (i32, [u32, vp, u64, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, C.POINTER(AssocStatsC)]),
        "dcrx_assoc_ranksum_device": (i32, [u32, u64, u32, u64, vp, vp, vp, vp, u32, vp, u32, u64, vp, vp, vp, vp, vp, vp]),
        "dcrx_assoc_ranksum": (i32, [u32, u64, u32, u64, vp, vp, vp, vp, u32, vp, u32, u64, vp, vp, vp, vp, vp, C.POINTER(AssocRanksumStatsC)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the .so does not match include/dcrx.h
        fn.restype = res
        fn.argtypes = args
    if L.dcrx_abi_version() != ABI_VERSION:
        raise ImportError(f"libdcrx.so ABI {L.dcrx_abi_version()} != binding {ABI_VERSION}: rebuild")
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise DcrxError(rc, lib().dcrx_last_error().decode("utf-8", "replace"))
    return rc


def _strs(xs):
    arr = (C.c_char_p * max(1, len(xs)))()
    for i, x in enumerate(xs):
        arr[i] = x.encode("ascii") if isinstance(x, str) else bytes(x)
    return arr


class Tables:
    """Opaque dcrx_tables_t: replaces import_tcr_info's module globals
    (reference decombine.py:593-746) for one chain."""

    def __init__(self, v_tags, v_jumps, v_regions, j_tags, j_jumps, j_regions,
                 v_half_split: int, j_half_split: int):
        if not (len(v_tags) == len(v_jumps) == len(v_regions)):
            raise ValueError("V tags, jumps and regions differ in length")
        if not (len(j_tags) == len(j_jumps) == len(j_regions)):
            raise ValueError("J tags, jumps and regions differ in length")
        self._keep = (_strs(v_tags), (C.c_int32 * max(1, len(v_jumps)))(*[int(x) for x in v_jumps]),
                      _strs(v_regions), _strs(j_tags),
                      (C.c_int32 * max(1, len(j_jumps)))(*[int(x) for x in j_jumps]), _strs(j_regions))
        ts = TagSetC(len(v_tags), self._keep[0], self._keep[1], self._keep[2],
                     len(j_tags), self._keep[3], self._keep[4], self._keep[5],
                     int(v_half_split), int(j_half_split))
        h = C.c_void_p()
        self._h = None
        check(lib().dcrx_tables_create(C.byref(ts), C.byref(h)))
        self._h = h
        self.n_v, self.n_j = len(v_tags), len(j_tags)
        # what a receiver of narrow tuples re-derives positions from (TupleCodec)
        self.v_jumps = [int(x) for x in v_jumps]
        self.j_jumps = [int(x) for x in j_jumps]
        self.j_lens = [len(x) for x in j_tags]
        self.j_half_split = int(j_half_split)

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        inf = TablesInfoC()
        check(lib().dcrx_tables_info(self._h, C.byref(inf)))
        return {"n_v": inf.n_v, "n_j": inf.n_j, "n_states": inf.n_states, "dfa_bytes": inf.dfa_bytes,
                "n_keywords": list(inf.n_keywords), "max_tag_len": inf.max_tag_len,
                "tables_in_lds": bool(inf.tables_in_lds),
                "equal_len_per_automaton": bool(inf.equal_len_per_automaton), "pair_scan_bytes": inf.pair_scan_bytes,
                "v2_tables": bool(inf.v2_tables), "v2_states": list(inf.v2_states), "v2_scan_bytes": max(inf.v2_scan_bytes),
                "max_read_len": inf.max_read_len}

    def tune_state(self, n_reads: int, orientation: str = "reverse") -> dict:
        """dcrx_tune_state: what the handle has settled for the finishing launches of batches of n_reads' size class."""
        st = TuneStateC()
        check(lib().dcrx_tune_state(self._h, ORIENTATIONS[orientation], int(n_reads), C.byref(st)))
        first, second = int(st.candidates) & 0xFFFF, int(st.candidates) >> 16
        return {"rescue_waves": int(st.rescue_waves), "launches": int(st.launches), f"us_{first}": round(float(st.us_first), 2),
                f"us_{second}": round(float(st.us_second), 2),
                "launch_form": {0: "none yet", 1: "three-launch form", 2: "v2, tail as a role", 3: "v2, tail inside the scan", 4: "v2, tail and list E inside the scan"}.get(int(st.launch_form), "?")}

    def close(self):
        if self._h is not None:
            lib().dcrx_tables_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stride_for(max_len: int) -> int:
    """Smallest legal stride (multiple of 8 bytes) for reads of up to max_len nt."""
    return max(8, ((max_len + 3) // 4 + 7) // 8 * 8)


class PackedBatch:
    """Host-side packed reads (what dcrx_pack_reads produces)."""

    def __init__(self, packed, stride, read_len, lens, exc_read, exc_pos, exc_chr):
        self.packed = packed
        self.stride = int(stride)
        self.read_len = int(read_len)
        self.lens = lens
        self.exc_read, self.exc_pos, self.exc_chr = exc_read, exc_pos, exc_chr

    @property
    def n_reads(self) -> int:
        return self.packed.shape[0]

    def as_c(self) -> BatchC:
        b = BatchC()
        b.n_reads = self.n_reads
        b.packed = self.packed.ctypes.data
        b.stride = self.stride
        b.read_len = self.read_len
        b.lens = self.lens.ctypes.data if self.lens is not None else None
        b.n_exc = len(self.exc_read)
        b.exc_read = self.exc_read.ctypes.data if len(self.exc_read) else None
        b.exc_pos = self.exc_pos.ctypes.data if len(self.exc_read) else None
        b.exc_chr = self.exc_chr.ctypes.data if len(self.exc_read) else None
        return b


def pack_reads(reads, stride: int | None = None) -> PackedBatch:
    """Packs a list of str/bytes reads (or a (buffer, offsets) pair) 2 bits per base."""
    if isinstance(reads, tuple):
        buf, offsets = reads
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    else:
        bs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
        offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        buf = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, dtype=np.uint8)
    n = len(offsets) - 1
    lens64 = np.diff(offsets.astype(np.int64)) if n else np.zeros(0, dtype=np.int64)
    max_len = int(lens64.max()) if n else 0
    if stride is None:
        stride = stride_for(max_len)
    packed = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    cap = 1024
    while True:
        er = np.zeros(cap, dtype=np.uint32)
        ep = np.zeros(cap, dtype=np.uint16)
        ec = np.zeros(cap, dtype=np.uint8)
        got = lib().dcrx_pack_reads(buf.ctypes.data if len(buf) else None, offsets.ctypes.data, n, stride,
                                    packed.ctypes.data if n else None, lens.ctypes.data, er.ctypes.data,
                                    ep.ctypes.data, ec.ctypes.data, cap)
        check(int(got))
        if got <= cap:
            break
        cap = int(got)
    uniform = n > 0 and bool((lens64 == lens64[0]).all())
    return PackedBatch(packed, stride, int(lens64[0]) if uniform else 0, None if uniform else lens,
                       er[:got].copy(), ep[:got].copy(), ec[:got].copy())


def pack_reads_span(text, start, length, stride: int | None = None) -> PackedBatch:
    """Packs the reads text[start[r] : start[r]+length[r]] (bytes / uint8 buffer, uint64, uint32)."""
    buf = text if isinstance(text, np.ndarray) else np.frombuffer(text, dtype=np.uint8)
    start = np.ascontiguousarray(start, dtype=np.uint64)
    length = np.ascontiguousarray(length, dtype=np.uint32)
    n = len(start)
    max_len = int(length.max()) if n else 0
    if stride is None:
        stride = stride_for(max_len)
    packed = np.empty((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    cap = 1024 + n // 64
    while True:
        er = np.zeros(cap, dtype=np.uint32)
        ep = np.zeros(cap, dtype=np.uint16)
        ec = np.zeros(cap, dtype=np.uint8)
        got = lib().dcrx_pack_reads_span(buf.ctypes.data if len(buf) else None, start.ctypes.data, length.ctypes.data, n,
                                         stride, packed.ctypes.data if n else None, lens.ctypes.data, er.ctypes.data,
                                         ep.ctypes.data, ec.ctypes.data, cap)
        check(int(got))
        if got <= cap:
            break
        cap = int(got)
    uniform = n > 0 and bool((length == length[0]).all())
    return PackedBatch(packed, stride, int(length[0]) if uniform else 0, None if uniform else lens,
                       er[:got].copy(), ep[:got].copy(), ec[:got].copy())


NO_QUAL = 0xFFFFFFFF
FAST_MAX_READ_LEN = 511      # reads up to this length run on the register shapes; longer ones (to dcrx_tables_info.max_read_len) in batches of their own


class FastqBatch:
    """One batch of records from FastqReader: `text` (bytes) plus offset / length arrays
    (qual_len == NO_QUAL where the reference's readfq yields qual None)."""

    __slots__ = ("n", "text", "name_off", "name_len", "seq_off", "seq_len", "qual_off", "qual_len")

    def __init__(self, c: FastqBatchC, copy: bool = True):
        n = self.n = int(c.n_records)
        # zero-copy window on the reader's buffer: valid until the next call of next() on that reader
        self.text = (C.c_char * int(c.text_bytes)).from_address(c.text) if c.text_bytes else b""

        def arr(ptr, ct, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,))
            # copy=False: the offset and length arrays are windows on the reader's store as well (36 MB per million records not
            # copied) — valid, like the text, until the next call of next() on that reader
            return a.astype(dt, copy=True) if copy else a
        self.name_off, self.name_len = arr(c.name_off, C.c_uint64, np.uint64), arr(c.name_len, C.c_uint32, np.uint32)
        self.seq_off, self.seq_len = arr(c.seq_off, C.c_uint64, np.uint64), arr(c.seq_len, C.c_uint32, np.uint32)
        self.qual_off, self.qual_len = arr(c.qual_off, C.c_uint64, np.uint64), arr(c.qual_len, C.c_uint32, np.uint32)

    def truncate(self, n: int) -> None:
        self.n = n
        for a in ("name_off", "name_len", "seq_off", "seq_len", "qual_off", "qual_len"):
            setattr(self, a, getattr(self, a)[:n])

    def name(self, k: int) -> str:
        o = int(self.name_off[k])
        return self.text[o:o + int(self.name_len[k])].decode("utf-8", "replace")

    def seq(self, k: int) -> str:
        o = int(self.seq_off[k])
        return self.text[o:o + int(self.seq_len[k])].decode("latin-1")

    def qual(self, k: int):
        if int(self.qual_len[k]) == NO_QUAL:
            return None
        o = int(self.qual_off[k])
        return self.text[o:o + int(self.qual_len[k])].decode("latin-1")

    def records(self):
        """(name, seq, qual) tuples, as readfq yields them."""
        return [(self.name(k), self.seq(k), self.qual(k)) for k in range(self.n)]


class FastqReader:
    """Batch FASTQ / FASTA reader in libdcrx (dcrx_fastq_*): same records as readfq()."""

    def __init__(self, path: str, gzipped: bool | None = None, byte_range=None):
        """byte_range = (begin, end): the records of that byte range of a plain four-line FASTQ file only (a shard)."""
        if gzipped is None:
            gzipped = str(path).endswith(".gz")
        self._h = C.c_void_p()
        if byte_range is not None:
            check(lib().dcrx_fastq_open_range(os.fsencode(path), int(byte_range[0]), int(byte_range[1]), C.byref(self._h)))
        else:
            check(lib().dcrx_fastq_open(os.fsencode(path), int(bool(gzipped)), C.byref(self._h)))

    def next(self, max_records: int, copy: bool = True) -> FastqBatch:
        c = FastqBatchC()
        check(lib().dcrx_fastq_next(self._h, int(max_records), C.byref(c)))
        return FastqBatch(c, copy)

    def close(self) -> None:
        if self._h:
            lib().dcrx_fastq_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fastq_lines(path: str, begin: int, end: int, nth: int = 0, count: bool = True):
    """(newlines in the bytes [begin, end) of the file, offset just behind the nth of them or None, a carriage return occurs,
    file size) — dcrx_fastq_lines; count=False: only the offset (the scan stops at the nth newline)."""
    n, off, cr, size = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_uint64(0)
    check(lib().dcrx_fastq_lines(os.fsencode(path), int(begin), int(end), int(nth), C.byref(n) if count else None, C.byref(off), C.byref(cr),
                                 C.byref(size)))
    return int(n.value), (None if off.value == 0xFFFFFFFFFFFFFFFF else int(off.value)), bool(cr.value), int(size.value)


def count_prefix_byte(text: bytes, start, length, prefix: int, byte: str) -> int:
    start = np.ascontiguousarray(start, dtype=np.uint64)
    length = np.ascontiguousarray(length, dtype=np.uint32)
    if len(start) == 0 or prefix <= 0:
        return 0
    buf = np.frombuffer(text, dtype=np.uint8)
    return int(lib().dcrx_count_prefix_byte(buf.ctypes.data, start.ctypes.data, length.ctypes.data, len(start),
                                            int(prefix), ord(byte)))


class SeparatorClash(RuntimeError):
    """A row field contains the field separator byte: the caller assembles that batch row by row."""


def _uninitialised_bytes(n: int) -> bytes:
    """A bytes object of n bytes that nobody has written yet (CPython: PyBytes_FromStringAndSize(NULL, n)); the caller fills
    it through _bytes_address() before anyone else sees it."""
    f = C.pythonapi.PyBytes_FromStringAndSize
    f.restype, f.argtypes = C.py_object, [C.c_char_p, C.c_ssize_t]
    return f(None, n)


def _bytes_address(b: bytes) -> int:
    f = C.pythonapi.PyBytes_AsString
    f.restype, f.argtypes = C.c_void_p, [C.py_object]
    return f(b)


def assemble_rows_blob(records, vdj, qual, ident, bc, bcq, tail=None, field_sep: str = ", "):
    """dcrx_assemble_rows: each argument after `records` is (text bytes, uint64 start[], uint32 len[]).
    Returns (bytes blob of '\n'-terminated rows, number of rows)."""
    keep = []

    def spans(t):
        if t is None:
            return None
        text, start, length = t
        buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
        start = np.ascontiguousarray(start, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        keep.extend((buf, start, length))
        return C.byref(SpansC(buf.ctypes.data, start.ctypes.data, length.ctypes.data))
    records = np.ascontiguousarray(records)
    args = [spans(t) for t in (vdj, qual, ident, bc, bcq, tail)]
    nrows = C.c_uint64(0)
    sep = field_sep.encode("latin-1")
    need = int(lib().dcrx_assemble_rows(records.ctypes.data, len(records), *args, sep, None, 0, C.byref(nrows)))
    check(need)
    # the text as a bytes object whose buffer the library fills: bytearray(need) zeroes its half a gigabyte on one thread first
    # (0.24 s of a 0.37 s call for 4 M reads on the build container), a fresh bytes object's pages are first touched by the
    # library's sixteen writers
    out = _uninitialised_bytes(need)
    if need:
        got = int(lib().dcrx_assemble_rows(records.ctypes.data, len(records), *args, sep, _bytes_address(out), need,
                                           C.byref(nrows)))
        if got == -2:                   # DCRX_E_UNSUPPORTED
            raise SeparatorClash(lib().dcrx_last_error().decode("utf-8", "replace"))
        check(got)
        if got != need:
            raise DcrxError(-1, f"dcrx_assemble_rows wrote {got} of {need} bytes")
    return out, int(nrows.value)


def unpack_reads_raw(batch: PackedBatch):
    """Inverse of pack_reads into one ASCII buffer: (uint8 buffer with a trailing NUL, uint64 offsets[n+1])."""
    n = batch.n_reads
    lens = batch.lens.astype(np.uint64) if batch.lens is not None else np.full(n, batch.read_len, dtype=np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    out = np.zeros(int(offsets[-1]) + 1, dtype=np.uint8)
    b = batch.as_c()
    check(lib().dcrx_unpack_reads(C.byref(b), offsets.ctypes.data, out.ctypes.data))
    return out, offsets


def unpack_reads(batch: PackedBatch):
    """Inverse of pack_reads: list of str."""
    n = batch.n_reads
    lens = batch.lens.astype(np.uint64) if batch.lens is not None else np.full(n, batch.read_len, dtype=np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    out = np.zeros(int(offsets[-1]) + 1, dtype=np.uint8)
    b = batch.as_c()
    check(lib().dcrx_unpack_reads(C.byref(b), offsets.ctypes.data, out.ctypes.data))
    raw = out.tobytes()
    return [raw[int(offsets[i]):int(offsets[i + 1])].decode("latin-1") for i in range(n)]


def make_cfg(orientation="reverse", allow_ns=False, lenthreshold=130, flags=0) -> CfgC:
    o = ORIENTATIONS[orientation] if isinstance(orientation, str) else int(orientation)
    return CfgC(o, int(bool(allow_ns)), int(lenthreshold), int(flags))


class GzipWriter:
    """dcrx_gzip_open / write / close: a gzip file written by several threads (multi-member; any gzip reader reads it as one
    stream).  Stands for the reference's `gzip.open(name, "wt")` + writelines (io.py:497-506)."""

    def __init__(self, path: str, level: int = 6, n_threads: int = 0):
        self._h = C.c_void_p()
        check(lib().dcrx_gzip_open(os.fsencode(path), int(level), int(n_threads), C.byref(self._h)))

    def write(self, data) -> None:
        mv = memoryview(data).cast("B")
        if mv.nbytes:
            arr = np.frombuffer(mv, dtype=np.uint8)
            check(lib().dcrx_gzip_write(self._h, arr.ctypes.data, mv.nbytes))

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, C.c_void_p()
            check(lib().dcrx_gzip_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PinnedBlock:
    """Page-locked host memory from dcrx_malloc_host, freed with the last array that views it."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        check(lib().dcrx_malloc_host(C.byref(self.ptr), max(1, int(nbytes))))
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().dcrx_free_host(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype) -> np.ndarray:
    """An uninitialised numpy array in page-locked host memory: dcrx_decombine copies from / into such buffers directly."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    blk = _PinnedBlock(n)
    buf = (C.c_uint8 * max(1, n)).from_address(blk.ptr.value)
    buf._dcrx_block = blk           # the ctypes object, which the array keeps alive, keeps the block alive
    return np.frombuffer(buf, dtype=np.uint8, count=n).view(dtype).reshape(shape)


def _host_call(tables_list, batch: PackedBatch, cfg: CfgC, recs=None, counts_list=None, first_index: int = 0, index=None,
               chains: bool = True) -> list:
    """The host-buffer entries over tables_list: records into recs (a records array per chain), or DCRs into counts_list
    (a DcrCounts per chain) read r as ordinal first_index + r (or first_index + index[r]).  The chains entry, or with
    chains=False the single-chain entry over the one chain.  Returns the counters (uint64[32]) per chain."""
    L, k = lib(), max(1, len(tables_list))
    cnts = [np.zeros(N_COUNTERS, dtype=np.uint64) for _ in tables_list]
    handles = (C.c_void_p * k)(*[t.handle for t in tables_list])
    cnt_ptrs = (C.c_void_p * k)(*[c.ctypes.data for c in cnts])
    cfg_p, b = C.byref(cfg), batch.as_c()
    if counts_list is None:
        rec_ptrs = (C.c_void_p * k)(*[r.ctypes.data if batch.n_reads else None for r in recs])
        rc = (L.dcrx_decombine_chains(handles, len(tables_list), cfg_p, C.byref(b), rec_ptrs, cnt_ptrs) if chains else
              L.dcrx_decombine(handles[0], cfg_p, C.byref(b), rec_ptrs[0], cnt_ptrs[0]))
    else:
        idx, idx_ptr = _index_arg(index, batch.n_reads)
        counts_h = (C.c_void_p * k)(*[c.handle for c in counts_list])
        rc = (L.dcrx_decombine_chains_count(handles, len(tables_list), cfg_p, C.byref(b), counts_h, int(first_index), idx_ptr,
                                            cnt_ptrs) if chains else
              L.dcrx_decombine_count(handles[0], cfg_p, C.byref(b), counts_h[0], int(first_index), idx_ptr, cnt_ptrs[0]))
    check(rc)
    return cnts


def decombine(tables: Tables, batch: PackedBatch, orientation="reverse", allow_ns=False,
              lenthreshold=130, flags=0, out: np.ndarray | None = None):
    """dcrx_decombine on host buffers.  Returns (records[RECORD_DTYPE], counters uint64[32]).  `out`: a records array to
    fill (e.g. pinned_empty(n, RECORD_DTYPE), reused from call to call)."""
    cfg = make_cfg(orientation, allow_ns, lenthreshold, flags)
    if out is not None:
        assert out.dtype == RECORD_DTYPE and out.shape == (batch.n_reads,) and out.flags.c_contiguous
    rec = out if out is not None else np.zeros(batch.n_reads, dtype=RECORD_DTYPE)
    return rec, _host_call([tables], batch, cfg, recs=[rec], chains=False)[0]


MAX_CHAINS = 4          # DCRX_MAX_CHAINS


def decombine_chains(tables_list, batch: PackedBatch, orientation="reverse", allow_ns=False, lenthreshold=130, flags=0):
    """dcrx_decombine_chains: one host batch, uploaded once, resolved against every chain's tables.  Returns
    [(records[RECORD_DTYPE], counters uint64[32]), ...] in the order of `tables_list`; each pair equals what decombine()
    gives for that chain alone."""
    tables_list = list(tables_list)
    cfg = make_cfg(orientation, allow_ns, lenthreshold, flags)
    recs = [np.zeros(batch.n_reads, dtype=RECORD_DTYPE) for _ in tables_list]
    return list(zip(recs, _host_call(tables_list, batch, cfg, recs=recs)))


class DcrCounts:
    """Opaque dcrx_counts_t: the distinct DCRs (v, j, vdel, jdel, insert) of the barcode-free stage with their read counts,
    in a table on the device that grows across calls (replaces the reference's `Counter` over dcr() results,
    decombine.py:1041-1060)."""

    def __init__(self):
        h = C.c_void_p()
        self._h = None
        check(lib().dcrx_counts_create(C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def reset(self):
        check(lib().dcrx_counts_reset(self._h))

    def set_hash_bits(self, bits: int):
        """dcrx_counts_set_hash_bits (tests): keys keep `bits` hash bits, so that distinct DCRs collide; same results."""
        check(lib().dcrx_counts_set_hash_bits(self._h, int(bits)))

    def read(self) -> dict:
        """dcrx_counts_read: the distinct DCRs in Counter.most_common() order — arrays v, j, vdel, jdel, count, first (the
        first read's ordinal), ins_off (n + 1) and the inserts' text `ins_text` (bytes)."""
        tb = C.c_uint64(0)
        n = check(int(lib().dcrx_counts_read(self._h, None, None, None, None, None, None, None, None, 0, 0, C.byref(tb))))
        out = {"v": np.zeros(n, np.uint16), "j": np.zeros(n, np.uint16), "vdel": np.zeros(n, np.uint8),
               "jdel": np.zeros(n, np.uint8), "count": np.zeros(n, np.uint64), "first": np.zeros(n, np.uint64),
               "ins_off": np.zeros(n + 1, np.uint64)}
        text = np.zeros(max(1, int(tb.value)), np.uint8)
        got = check(int(lib().dcrx_counts_read(self._h, *[out[k].ctypes.data for k in ("v", "j", "vdel", "jdel", "count", "first", "ins_off")],
                                                text.ctypes.data, n, len(text), C.byref(tb))))
        if got != n:
            raise DcrxError(-1, "dcrx_counts_read: the number of distinct DCRs changed between two calls")
        out["ins_text"] = text[:int(tb.value)].tobytes()
        return out

    def close(self):
        if self._h is not None:
            lib().dcrx_counts_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def count_rows(counted: dict) -> list:
    """The six-field rows [v, j, vdel, jdel, insert, count] of what DcrCounts.read() gives (the first five as the `.n12` row
    holds them, text; the count an int)."""
    text, off = counted["ins_text"], counted["ins_off"]
    return [[str(int(counted["v"][k])), str(int(counted["j"][k])), str(int(counted["vdel"][k])), str(int(counted["jdel"][k])),
             text[int(off[k]):int(off[k + 1])].decode("latin-1"), int(counted["count"][k])] for k in range(len(counted["v"]))]


COUNTS_LINE_BOUND = 54      # DCRX_COUNTS_LINE_BOUND


def format_counts(counted: dict, field_sep: str = ", ") -> bytes:
    """dcrx_format_counts: the `.nbc` text of what DcrCounts.read() gives, one "v, j, vdel, jdel, insert, count" line per DCR."""
    n = len(counted["v"])
    arrs = [np.ascontiguousarray(counted[k]) for k in ("v", "j", "vdel", "jdel", "count", "ins_off")]
    text = np.frombuffer(counted["ins_text"], np.uint8) if counted["ins_text"] else np.zeros(1, np.uint8)
    sep = field_sep.encode("latin-1")
    args = [n] + [a.ctypes.data for a in arrs] + [text.ctypes.data, sep]
    # a buffer that always fits (DCRX_COUNTS_LINE_BOUND): the library writes it in one pass
    bound = n * (COUNTS_LINE_BOUND + 5 * len(sep)) + len(counted["ins_text"])
    out = _uninitialised_bytes(max(1, bound))
    got = check(int(lib().dcrx_format_counts(*args, _bytes_address(out), max(1, bound))))
    if got > bound:
        raise DcrxError(-1, f"dcrx_format_counts needs {got} bytes, more than the {bound} bound")
    return out[:got]


def merged_counts(counted: dict, order, count, first) -> dict:
    """dcrx_merge_gather: the table of the roots — entry m is input entry order[m] with the tree's count[m] and first[m] (the
    dict of arrays DcrCounts.read() gives, so NbcRows and format_counts take it as they take a counted table)."""
    order = np.ascontiguousarray(order, dtype=np.uint32)
    n, m = len(counted["v"]), len(order)
    src = [np.ascontiguousarray(counted[k], dtype=t) for k, t in (("v", np.uint16), ("j", np.uint16), ("vdel", np.uint8),
                                                                   ("jdel", np.uint8), ("ins_off", np.uint64))]
    text = np.frombuffer(counted["ins_text"], np.uint8) if counted["ins_text"] else np.zeros(1, np.uint8)
    out = {"v": np.zeros(m, np.uint16), "j": np.zeros(m, np.uint16), "vdel": np.zeros(m, np.uint8), "jdel": np.zeros(m, np.uint8),
           "count": np.array(count, np.uint64), "first": np.array(first, np.uint64), "ins_off": np.zeros(m + 1, np.uint64)}
    new_text = np.zeros(max(1, len(counted["ins_text"])), np.uint8)
    got = check(int(lib().dcrx_merge_gather(n, m, order.ctypes.data, *[a.ctypes.data for a in src], text.ctypes.data,
                                            *[out[k].ctypes.data for k in ("v", "j", "vdel", "jdel", "ins_off")],
                                            new_text.ctypes.data)))
    out["ins_text"] = new_text[:got].tobytes()
    return out


def merge_dcrs(tables: "Tables", counted: dict, distance: int = 1, ratio: int = 10):
    """dcrx_merge_dcrs on the current device: the counted table (what DcrCounts.read() gives) with every erroneous DCR folded
    into its root — (merged table, statistics dict over MERGE_STATS, root_of: the rank of every input entry's root)."""
    n = len(counted["v"])
    arrs = [np.ascontiguousarray(counted[k], dtype=t) for k, t in (("v", np.uint16), ("j", np.uint16), ("vdel", np.uint8),
                                                                    ("jdel", np.uint8), ("count", np.uint64), ("first", np.uint64),
                                                                    ("ins_off", np.uint64))]
    text = np.frombuffer(counted["ins_text"], np.uint8) if counted["ins_text"] else np.zeros(1, np.uint8)
    root_of, order = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cnt, fst = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    st = MergeStatsC()
    m = check(int(lib().dcrx_merge_dcrs(tables.handle, n, *[a.ctypes.data for a in arrs], text.ctypes.data, int(distance),
                                        int(ratio), root_of.ctypes.data, order.ctypes.data, cnt.ctypes.data, fst.ctypes.data,
                                        C.byref(st))))
    stats = {k: int(getattr(st, k)) for k in MERGE_STATS}
    return merged_counts(counted, order[:m], cnt[:m], fst[:m]), stats, root_of


def call_groups(names) -> np.ndarray:
    """One call group per gene: genes whose names up to the '*' are equal (the .tsv's v_call / j_call) share a group."""
    seen: dict = {}
    return np.array([seen.setdefault(str(x).split("*")[0], len(seen)) for x in names], dtype=np.uint32)


class ClonoGenes:
    """dcrx_clono_genes_t: the gene set of the clonotype step — the tables of a Cdr3Genes, compiled and uploaded once, with the
    genes' names (their call groups, and the calls the file shows)."""

    def __init__(self, genes: Cdr3Genes, v_names, j_names):
        if len(v_names) != genes.n_v or len(j_names) != genes.n_j:
            raise ValueError("one name per gene")
        self.cdr3 = genes
        self.v_calls, self.j_calls = ([str(x).split("*")[0] for x in names] for names in (v_names, j_names))
        self.v_group, self.j_group = call_groups(v_names), call_groups(j_names)
        h = C.c_void_p()
        check(lib().dcrx_clono_genes_create(C.byref(genes.c), self.v_group.ctypes.data, self.j_group.ctypes.data, C.byref(h)))
        self.handle = h

    def set_hash_bits(self, bits: int) -> None:
        check(lib().dcrx_clono_set_hash_bits(self.handle, int(bits)))

    def close(self):
        if getattr(self, "handle", None):
            lib().dcrx_clono_genes_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _entry_arrays(counted: dict):
    """(v, j, vdel, jdel as int32, count, ins_off as uint64, the inserts' bytes as uint8) of a counted table."""
    ints = [np.ascontiguousarray(counted[k], dtype=np.int32) for k in ("v", "j", "vdel", "jdel")]
    cnt, off = (np.ascontiguousarray(counted[k], dtype=np.uint64) for k in ("count", "ins_off"))
    text = np.frombuffer(counted["ins_text"], np.uint8) if counted["ins_text"] else np.zeros(1, np.uint8)
    return ints, cnt, off, text


def clono_row_fields(rows: np.ndarray, j_pos=None) -> np.ndarray:
    """The fields dcrx_clono_row_t shares with dcrx_cdr3_row_t, spelled out as include/dcrx.h derives them (CDR3_ROW_DTYPE;
    seq_off / aa_off stay 0).  j_pos: the J gene's position per row, for the motif window of MOTIF_LEFT rows."""
    out = np.zeros(len(rows), dtype=CDR3_ROW_DTYPE)
    for k, r in enumerate(rows):
        o = out[k]
        o["status"] = r["status"]
        if r["status"] == CDR3_BAD_CODON:
            o["bad_codon_at"] = int(r["start_cdr3"]) & 0xFFFFFFFF
        if r["status"] not in (CDR3_OK, CDR3_MOTIF_LEFT):
            continue
        fl = int(r["flags"])
        for bit, name in enumerate(("productive", "in_frame", "stop", "conserved_c", "conserved_f")):
            o[name] = (fl >> bit) & 1
        sn, start, end = int(r["seq_len"]), int(r["start_cdr3"]), int(r["end_cdr3"])
        o["seq_len"], o["aa_len"], o["start_cdr3"], o["end_cdr3"] = sn, sn // 3, start, end
        if r["status"] == CDR3_MOTIF_LEFT:
            lo, hi, _ = slice(start, None).indices(sn // 3)
            jp = int(j_pos[k])
            a, b, _ = slice(jp, jp + 4).indices(max(0, hi - lo))
            o["junction_aa_off"], o["junction_aa_len"] = lo + a, max(0, b - a)
        elif fl & 1:
            lo, hi, _ = slice(start, end).indices(sn // 3)
            o["junction_aa_off"], o["junction_aa_len"] = lo, max(0, hi - lo)
            lo, hi, _ = slice(3 * start, 3 * end).indices(sn)
            o["junction_off"], o["junction_len"] = lo, max(0, hi - lo)
    return out


def clono_work_bytes(n: int, text_bytes: int) -> int:
    return int(lib().dcrx_clono_work_bytes(int(n), int(text_bytes)))


def cdr3_device(genes: ClonoGenes, n: int, d_v, d_j, d_vdel, d_jdel, d_ins_off, d_ins_text, text_bytes: int, d_rows, d_arena,
                arena_cap: int, d_arena_need, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_device: the calls of every entry of a table in HBM (DeviceBuffers), asynchronous on `stream`."""
    check(lib().dcrx_cdr3_device(genes.handle, int(n), d_v.ptr, d_j.ptr, d_vdel.ptr, d_jdel.ptr, d_ins_off.ptr,
                                 d_ins_text.ptr if d_ins_text is not None else None, int(text_bytes), d_rows.ptr,
                                 d_arena.ptr if d_arena is not None else None, int(arena_cap),
                                 d_arena_need.ptr if d_arena_need is not None else None, d_work.ptr, int(work_bytes), stream))


def clonotypes(genes: ClonoGenes, counted: dict):
    """dcrx_clonotypes on the current device: the counted table (v, j, vdel, jdel, count, ins_off, ins_text) grouped into
    clonotypes — (table, statistics dict over CLONOTYPE_STATS, clonotype_of).  table: rep (the representative's rank),
    duplicate_count, n_dcrs, top_dcr_count per row, and the rows' junction_aa / junction as junc_off (2 rows + 1) into
    junc_text."""
    ints, cnt, off, text = _entry_arrays(counted)
    n = len(ints[0])
    rep, nd, of = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    dup, top, joff = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(2 * n + 1, np.uint64)
    st = ClonotypeStatsC()
    m = check(int(lib().dcrx_clonotypes(genes.handle, n, *[a.ctypes.data for a in ints], cnt.ctypes.data, off.ctypes.data,
                                        text.ctypes.data, rep.ctypes.data, dup.ctypes.data, nd.ctypes.data, top.ctypes.data,
                                        joff.ctypes.data, of.ctypes.data, C.byref(st))))
    need = check(int(lib().dcrx_clonotypes_text(genes.handle, None, 0)))
    jtext = np.zeros(max(1, need), np.uint8)
    check(int(lib().dcrx_clonotypes_text(genes.handle, jtext.ctypes.data, need)))
    table = {"rep": rep[:m].copy(), "duplicate_count": dup[:m].copy(), "n_dcrs": nd[:m].copy(), "top_dcr_count": top[:m].copy(),
             "junc_off": joff[:2 * m + 1].copy(), "junc_text": jtext[:need].tobytes()}
    return table, {k: int(getattr(st, k)) for k in CLONOTYPE_STATS}, of


def format_clonotypes(genes: ClonoGenes, table: dict, counted: dict) -> bytes:
    """dcrx_format_clonotypes: the `.clonotypes.tsv` text of a clonotype table over the counted table it came from."""
    ints, _, off, text = _entry_arrays(counted)

    def blob(strings):
        bs = [x.encode("latin-1") for x in strings]
        o = np.zeros(len(bs) + 1, dtype=np.uint32)
        o[1:] = np.cumsum([len(b) for b in bs])
        return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy(), o
    (vc, vo), (jc, jo) = blob(genes.v_calls), blob(genes.j_calls)
    m = len(table["rep"])
    cols = [np.ascontiguousarray(table[k], dtype=t) for k, t in (("rep", np.uint32), ("duplicate_count", np.uint64), ("n_dcrs", np.uint32),
                                                                 ("top_dcr_count", np.uint64), ("junc_off", np.uint64))]
    jtext = np.frombuffer(table["junc_text"], np.uint8) if table["junc_text"] else np.zeros(1, np.uint8)
    args = [m] + [a.ctypes.data for a in cols] + [jtext.ctypes.data, len(ints[0])] + [a.ctypes.data for a in ints] + \
           [off.ctypes.data, text.ctypes.data, len(genes.v_calls), vc.ctypes.data, vo.ctypes.data, len(genes.j_calls), jc.ctypes.data,
            jo.ctypes.data]
    need = check(int(lib().dcrx_format_clonotypes(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(lib().dcrx_format_clonotypes(*args, _bytes_address(out), need)))
    return bytes(out[:need])


# ---- the CDR3 network (--cdr3-network): include/dcrx.h "the CDR3 network" ----

def cdr3_metric_code(metric) -> int:
    """DCRX_CDR3NET_HAMMING / _LEVENSHTEIN for a metric's name (None: hamming); a number is passed on as it is (the library
    refuses the ones it does not know)."""
    if metric is None:
        return 0
    if isinstance(metric, str):
        if metric not in CDR3_METRICS:
            raise ValueError(f"the CDR3 network's metric is one of {', '.join(CDR3_METRICS)}, not {metric!r}")
        return CDR3_METRICS[metric]
    return int(metric)


def cdr3net_work_bytes(m: int, text_bytes: int, metric=None) -> int:
    """dcrx_cdr3net_work_bytes, or with a metric dcrx_cdr3net_metric_work_bytes."""
    if metric is None:
        return int(lib().dcrx_cdr3net_work_bytes(int(m), int(text_bytes)))
    return int(lib().dcrx_cdr3net_metric_work_bytes(int(m), int(text_bytes), cdr3_metric_code(metric)))


def cdr3_neighbours_device(m: int, d_class, d_off, d_text, text_bytes: int, distance: int, d_degree, d_adj_off, d_adj, adj_cap: int,
                           d_adj_need, d_work, work_bytes: int, stream=None, metric=None):
    """dcrx_cdr3_neighbours_device (with a metric: dcrx_cdr3_neighbours_metric_device): degree and adjacency of every node of a
    table in HBM (DeviceBuffers), asynchronous on `stream`."""
    head = [int(m), d_class.ptr, d_off.ptr, d_text.ptr if d_text is not None else None, int(text_bytes), int(distance)]
    tail = [d_degree.ptr, d_adj_off.ptr, d_adj.ptr if d_adj is not None else None, int(adj_cap),
            d_adj_need.ptr if d_adj_need is not None else None, d_work.ptr, int(work_bytes), stream]
    if metric is None:
        check(lib().dcrx_cdr3_neighbours_device(*head, *tail))
    else:
        check(lib().dcrx_cdr3_neighbours_metric_device(*head, cdr3_metric_code(metric), *tail))


def _node_arrays(aa_off, aa_text):
    off = np.ascontiguousarray(aa_off, dtype=np.uint64)
    text = np.frombuffer(aa_text, np.uint8) if len(aa_text) else np.zeros(1, np.uint8)
    return off, text


def cdr3_network(classes, aa_off, aa_text: bytes, weights, distance: int, want_edges: bool = False, metric="hamming"):
    """dcrx_cdr3_network on the current device: m nodes (class, string = aa_text[aa_off[i]:aa_off[i + 1]], weight) linked where
    class and length agree and at most `distance` (1 or 2) bytes differ — or, with metric "levenshtein"
    (dcrx_cdr3_network_metric), where the class agrees and the strings are at most `distance` substitutions, insertions and
    deletions apart — (result, statistics dict over CDR3_NETWORK_STATS).
    result: degree and cluster_of per node; cluster_head, cluster_size and cluster_weight per cluster row (rows by head
    ascending); with want_edges the CSR adjacency adj_off (m + 1) and adj (a second call, once the first has sized it)."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    off, text = _node_arrays(aa_off, aa_text)
    m = len(cls)
    if len(off) != m + 1 or len(w) != m:
        raise ValueError("cdr3_network: one class and one weight per node, m + 1 offsets")
    if m >= CDR3NET_MAX_NODES:
        raise ValueError(f"the CDR3 network takes fewer than {CDR3NET_MAX_NODES:,} nodes, not {m:,}")
    deg, of, head, nn = (np.zeros(max(m, 1), np.uint32) for _ in range(4))
    cw = np.zeros(max(m, 1), np.uint64)
    adj_off = np.zeros(m + 1, np.uint64) if want_edges else None
    need = C.c_uint64(0)
    st = Cdr3NetworkStatsC()
    code = cdr3_metric_code(metric)

    def call(adj, cap):
        head_args = [m, cls.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data, int(distance)]
        tail_args = [deg.ctypes.data, of.ctypes.data, head.ctypes.data, nn.ctypes.data, cw.ctypes.data,
                     adj_off.ctypes.data if want_edges else None, adj.ctypes.data if adj is not None else None, cap, C.byref(need),
                     C.byref(st)]
        if code == 0:
            return check(int(lib().dcrx_cdr3_network(*head_args, *tail_args)))
        return check(int(lib().dcrx_cdr3_network_metric(*head_args, code, *tail_args)))
    c = call(None, 0)
    result = {"degree": deg[:m].copy(), "cluster_of": of[:m].copy(), "cluster_head": head[:c].copy(), "cluster_size": nn[:c].copy(),
              "cluster_weight": cw[:c].copy()}
    if want_edges:
        adj = np.zeros(max(1, need.value), np.uint32)
        if need.value:
            call(adj, need.value)
        result["adj_off"], result["adj"] = adj_off, adj[:need.value]
    return result, {k: int(getattr(st, k)) for k in CDR3_NETWORK_STATS}


def _calls_blob(strings):
    bs = [x.encode("latin-1") for x in strings]
    o = np.zeros(len(bs) + 1, dtype=np.uint32)
    o[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy(), o


def format_cdr3_clusters(v_idx, j_idx, v_calls, j_calls, aa_off, aa_text: bytes, weights, result: dict) -> bytes:
    """dcrx_format_cdr3_clusters: the `.cdr3_clusters.tsv` text — per node its rank, the calls v_calls[v_idx[i]] and
    j_calls[j_idx[i]], its string and weight, and its cluster's row, size and weight out of a cdr3_network result."""
    vi, ji = (np.ascontiguousarray(a, dtype=np.uint32) for a in (v_idx, j_idx))
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    off, text = _node_arrays(aa_off, aa_text)
    (vc, vo), (jc, jo) = _calls_blob(v_calls), _calls_blob(j_calls)
    cols = [np.ascontiguousarray(result[k], dtype=t) for k, t in (("cluster_of", np.uint32), ("cluster_size", np.uint32),
                                                                 ("cluster_weight", np.uint64), ("degree", np.uint32))]
    args = [len(vi), vi.ctypes.data, ji.ctypes.data, len(v_calls), vc.ctypes.data, vo.ctypes.data, len(j_calls), jc.ctypes.data,
            jo.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data, cols[0].ctypes.data, len(cols[1]), cols[1].ctypes.data,
            cols[2].ctypes.data, cols[3].ctypes.data]
    need = check(int(lib().dcrx_format_cdr3_clusters(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(lib().dcrx_format_cdr3_clusters(*args, _bytes_address(out), need)))
    return bytes(out[:need])


def format_cdr3_edges(aa_off, aa_text: bytes, result: dict, metric="hamming") -> bytes:
    """dcrx_format_cdr3_edges: the `.cdr3_edges.tsv` text of a cdr3_network result with edges; with metric "levenshtein"
    (dcrx_format_cdr3_edges_metric) the distance column is the Levenshtein distance and edges may join two lengths."""
    off, text = _node_arrays(aa_off, aa_text)
    adj_off = np.ascontiguousarray(result["adj_off"], dtype=np.uint64)
    adj = np.ascontiguousarray(result["adj"], dtype=np.uint32) if len(result["adj"]) else np.zeros(1, np.uint32)
    args = [len(off) - 1, adj_off.ctypes.data, adj.ctypes.data, off.ctypes.data, text.ctypes.data]
    code = cdr3_metric_code(metric)
    if code == 0:
        fmt = lib().dcrx_format_cdr3_edges
    else:
        fmt, args = lib().dcrx_format_cdr3_edges_metric, args + [code]
    need = check(int(fmt(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(fmt(*args, _bytes_address(out), need)))
    return bytes(out[:need])


# ---- match (the `match` sub-command): include/dcrx.h "match" ----

class Cdr3Index:
    """dcrx_cdr3_index_t: the targets (class, string = text[off[j]:off[j + 1]]) of a database, built on the current device once
    and kept there for any number of cdr3_match / cdr3_match_device calls, under either metric and every distance."""

    def __init__(self, classes, off, text: bytes):
        cls = np.ascontiguousarray(classes, dtype=np.uint32)
        o, t = _node_arrays(off, text)
        if len(o) != len(cls) + 1:
            raise ValueError("Cdr3Index: one class per target, m + 1 offsets")
        h = C.c_void_p()
        check(lib().dcrx_cdr3_index_create(len(cls), cls.ctypes.data, o.ctypes.data, t.ctypes.data, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        n, out, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().dcrx_cdr3_index_info(self._h, C.byref(n), C.byref(out), C.byref(b)))
        return {"targets": n.value, "out_of_reach": out.value, "device_bytes": b.value}

    def close(self):
        if getattr(self, "_h", None):
            lib().dcrx_cdr3_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cdr3_match_work_bytes(m_q: int, text_bytes: int, metric="hamming") -> int:
    """dcrx_cdr3_match_work_bytes."""
    return int(lib().dcrx_cdr3_match_work_bytes(int(m_q), int(text_bytes), cdr3_metric_code(metric)))


def cdr3_match_device(index: Cdr3Index, m_q: int, d_class, d_off, d_text, text_bytes: int, distance: int, d_degree, d_hit_off, d_hit,
                      hit_cap: int, d_hit_need, d_work, work_bytes: int, stream=None, metric="hamming"):
    """dcrx_cdr3_match_device: degree and hits of every query of a table in HBM (DeviceBuffers) against an index, asynchronous on
    `stream`."""
    def ptr(b):
        return b.ptr if b is not None else None
    check(lib().dcrx_cdr3_match_device(index.handle, int(m_q), ptr(d_class), ptr(d_off), ptr(d_text), int(text_bytes), int(distance),
                                       cdr3_metric_code(metric), ptr(d_degree), ptr(d_hit_off), ptr(d_hit), int(hit_cap), ptr(d_hit_need),
                                       ptr(d_work), int(work_bytes), stream))


def cdr3_match(index: Cdr3Index, classes, off, text: bytes, weights, distance: int, metric="hamming") -> dict:
    """dcrx_cdr3_match_run on the index's device, and everything it exports: m_q queries (class, string = text[off[i]:off[i + 1]],
    weight) against the index's targets; a hit is a query and a target of one class within `distance` (0, 1 or 2) under `metric`
    -> {"degree" per query, "hit_off" (m_q + 1) and "hit" (every query's targets ascending), "t_queries" and "t_weight" per
    target, "stats": dict over CDR3_MATCH_STATS}."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    o, t = _node_arrays(off, text)
    m = len(cls)
    if len(o) != m + 1 or len(w) != m:
        raise ValueError("cdr3_match: one class and one weight per query, m + 1 offsets")
    h = C.c_void_p()
    check(lib().dcrx_cdr3_match_run(index.handle, m, cls.ctypes.data, o.ctypes.data, t.ctypes.data, w.ctypes.data, int(distance),
                                    cdr3_metric_code(metric), C.byref(h)))
    return _cdr3_match_take(h, m, False)


def _cdr3_match_take(h, m: int, with_dist: bool) -> dict:
    """Everything a dcrx_cdr3_match_t exports, as cdr3_match returns it (with_dist: and "hit_dist"); releases the handle."""
    try:
        n_t, n_hits, st = C.c_uint64(0), C.c_uint64(0), Cdr3MatchStatsC()
        check(lib().dcrx_cdr3_match_info(h, None, C.byref(n_t), C.byref(n_hits), C.byref(st)))
        T, H = n_t.value, n_hits.value
        degree, hit, tq = np.zeros(max(m, 1), np.uint32), np.zeros(max(H, 1), np.uint32), np.zeros(max(T, 1), np.uint32)
        hit_off, tw = np.zeros(m + 1, np.uint64), np.zeros(max(T, 1), np.uint64)
        check(lib().dcrx_cdr3_match_export(h, degree.ctypes.data, hit_off.ctypes.data, hit.ctypes.data, tq.ctypes.data, tw.ctypes.data))
        dist = np.zeros(max(H, 1), np.uint32)
        if with_dist:
            check(lib().dcrx_cdr3_match_export_dist(h, dist.ctypes.data))
    finally:
        lib().dcrx_cdr3_match_destroy(h)
    out = {"degree": degree[:m], "hit_off": hit_off, "hit": hit[:H], "t_queries": tq[:T], "t_weight": tw[:T],
           "stats": {k: int(getattr(st, k)) for k in CDR3_MATCH_STATS}}
    if with_dist:
        out["hit_dist"] = dist[:H]
    return out


class Cdr3Cost:
    """dcrx_cdr3_cost_t: the weighted metric's cost — sub, a 32 x 32 uint8 table indexed by (byte & 31) of the two letters
    (symmetric, zero on the diagonal), gap (1 .. 255) and the trims (0 .. 16 each).  The constructor checks nothing: the
    library refuses what the contract refuses."""

    def __init__(self, sub, gap: int = 12, ntrim: int = 3, ctrim: int = 2):
        self.sub = np.ascontiguousarray(sub, dtype=np.uint8).reshape(32, 32).copy()
        self.gap, self.ntrim, self.ctrim = int(gap), int(ntrim), int(ctrim)

    @staticmethod
    def default_table() -> np.ndarray:
        """CDR3_COST_FAR between any two letters of A .. Z, CDR3_COST_NEAR's pairs below it, zero on the diagonal."""
        sub = np.zeros((32, 32), dtype=np.uint8)
        sub[1:27, 1:27] = CDR3_COST_FAR
        for cost, pairs in CDR3_COST_NEAR.items():
            for x, y in pairs:
                sub[ord(x) & 31, ord(y) & 31] = sub[ord(y) & 31, ord(x) & 31] = cost
        sub[np.arange(32), np.arange(32)] = 0
        return sub

    @classmethod
    def default(cls, gap: int = 12, ntrim: int = 3, ctrim: int = 2) -> "Cdr3Cost":
        return cls(cls.default_table(), gap, ntrim, ctrim)

    @classmethod
    def from_file(cls, path, gap: int = 12, ntrim: int = 3, ctrim: int = 2) -> "Cdr3Cost":
        """A tab-separated square table: the first row and the first column are single letters of A .. Z (the same letters in
        the same order; the corner cell is ignored), the cells integers 0 .. 255.  It covers the twenty amino acids, is
        symmetric and zero on its diagonal; a letter of A .. Z it lacks costs the file's largest cell against every other
        letter.  ValueError by line number for anything else."""
        with open(path, "rb") as fh:
            lines = fh.read().split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
        if not lines:
            raise ValueError(f"{path}, line 1: no header row")

        def letter(cell: bytes, n: int) -> int:
            if len(cell) != 1 or not b"A" <= cell <= b"Z":
                raise ValueError(f"{path}, line {n}: {cell.decode('latin-1')!r} is not a single letter A..Z")
            return cell[0] & 31
        cols = [letter(c, 1) for c in lines[0].split(b"\t")[1:]]
        if len(set(cols)) != len(cols):
            raise ValueError(f"{path}, line 1: a letter stands twice")
        missing = sorted(set(AMINO_ACIDS) - {chr(64 + c) for c in cols})
        if missing:
            raise ValueError(f"{path}, line 1: no column for {', '.join(missing)}")
        if len(lines) - 1 != len(cols):
            raise ValueError(f"{path}, line {len(lines)}: {len(lines) - 1} rows under {len(cols)} columns")
        cells = np.zeros((len(cols), len(cols)), dtype=np.int64)
        for r, line in enumerate(lines[1:]):
            n = r + 2
            f = line.split(b"\t")
            if len(f) != len(cols) + 1:
                raise ValueError(f"{path}, line {n}: {len(f)} fields, not {len(cols) + 1}")
            if letter(f[0], n) != cols[r]:
                raise ValueError(f"{path}, line {n}: row {f[0].decode('latin-1')} where the header has {chr(64 + cols[r])}")
            for k, cell in enumerate(f[1:]):
                if not cell.isdigit() or int(cell) > 255:
                    raise ValueError(f"{path}, line {n}: {cell.decode('latin-1')!r} is not an integer 0..255")
                cells[r, k] = int(cell)
        for r in range(len(cols)):
            if cells[r, r]:
                raise ValueError(f"{path}, line {r + 2}: the diagonal cell is {cells[r, r]}, not 0")
            for k in range(r):
                if cells[r, k] != cells[k, r]:
                    raise ValueError(f"{path}, line {r + 2}: {chr(64 + cols[r])}-{chr(64 + cols[k])} is {cells[r, k]} "
                                     f"but {chr(64 + cols[k])}-{chr(64 + cols[r])} is {cells[k, r]}")
        sub = np.zeros((32, 32), dtype=np.uint8)
        sub[1:27, 1:27] = cells.max()
        sub[np.ix_(cols, cols)] = cells
        sub[np.arange(32), np.arange(32)] = 0
        return cls(sub, gap, ntrim, ctrim)

    def as_c(self) -> Cdr3CostC:
        c = Cdr3CostC()
        C.memmove(c.sub, self.sub.ctypes.data, 1024)
        c.gap, c.ntrim, c.ctrim = (v & 0xFFFFFFFF for v in (self.gap, self.ntrim, self.ctrim))
        return c


def cdr3_match_weighted_work_bytes(m_q: int, text_bytes: int) -> int:
    """dcrx_cdr3_match_weighted_work_bytes."""
    return int(lib().dcrx_cdr3_match_weighted_work_bytes(int(m_q), int(text_bytes)))


def _radius(radius) -> int:
    if not 0 <= int(radius) < 1 << 32:
        raise ValueError(f"the radius is 0 .. {CDR3_MAX_RADIUS}, not {radius}")
    return int(radius)


def cdr3_match_weighted_device(index: Cdr3Index, m_q: int, d_class, d_off, d_text, text_bytes: int, cost: Cdr3Cost, radius: int, d_degree,
                               d_hit_off, d_hit, d_hit_dist, hit_cap: int, d_hit_need, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_match_weighted_device: cdr3_match_device under the weighted metric; d_hit_dist (may be None) receives the
    hits' distances."""
    def ptr(b):
        return b.ptr if b is not None else None
    c = cost.as_c() if cost is not None else None      # (alive across the call, which copies it)
    check(lib().dcrx_cdr3_match_weighted_device(index.handle, int(m_q), ptr(d_class), ptr(d_off), ptr(d_text), int(text_bytes),
                                                C.addressof(c) if c is not None else None, _radius(radius), ptr(d_degree),
                                                ptr(d_hit_off), ptr(d_hit), ptr(d_hit_dist), int(hit_cap), ptr(d_hit_need), ptr(d_work),
                                                int(work_bytes), stream))


def cdr3_match_weighted(index: Cdr3Index, classes, off, text: bytes, weights, cost: Cdr3Cost, radius: int) -> dict:
    """dcrx_cdr3_match_weighted_run: cdr3_match under the weighted metric — a hit is a query and a target of one class, both of
    1 .. 32 letters A .. Z, whose weighted distance under `cost` is at most `radius` -> cdr3_match's dict and "hit_dist", the
    distance of every hit as the device computed it."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    o, t = _node_arrays(off, text)
    m = len(cls)
    if len(o) != m + 1 or len(w) != m:
        raise ValueError("cdr3_match_weighted: one class and one weight per query, m + 1 offsets")
    h = C.c_void_p()
    c = cost.as_c() if cost is not None else None
    check(lib().dcrx_cdr3_match_weighted_run(index.handle, m, cls.ctypes.data, o.ctypes.data, t.ctypes.data, w.ctypes.data,
                                             C.addressof(c) if c is not None else None, _radius(radius), C.byref(h)))
    return _cdr3_match_take(h, m, True)


def _u32(value, what: str) -> int:
    if not 0 <= int(value) < 1 << 32:
        raise ValueError(f"{what} does not fit 32 bits: {value}")
    return int(value)


def cdr3_profile_weighted_work_bytes(m_q: int, text_bytes: int, bins: int) -> int:
    """dcrx_cdr3_profile_weighted_work_bytes."""
    return int(lib().dcrx_cdr3_profile_weighted_work_bytes(int(m_q), int(text_bytes), _u32(bins, "bins")))


def cdr3_profile_weighted_device(index: Cdr3Index, m_q: int, d_class, d_off, d_text, text_bytes: int, cost: Cdr3Cost, step: int, bins: int,
                                 d_profile, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_profile_weighted_device: per query of a table in HBM (DeviceBuffers) the histogram of its targets' weighted
    distances, m_q * bins dwords into d_profile, asynchronous on `stream`."""
    def ptr(b):
        return b.ptr if b is not None else None
    c = cost.as_c() if cost is not None else None      # (alive across the call, which copies it)
    check(lib().dcrx_cdr3_profile_weighted_device(index.handle, int(m_q), ptr(d_class), ptr(d_off), ptr(d_text), int(text_bytes),
                                                  C.addressof(c) if c is not None else None, _u32(step, "step"), _u32(bins, "bins"),
                                                  ptr(d_profile), ptr(d_work), int(work_bytes), stream))


def cdr3_profile_weighted(index: Cdr3Index, classes, off, text: bytes, cost: Cdr3Cost, step: int, bins: int) -> dict:
    """dcrx_cdr3_profile_weighted: m_q queries (class, string = text[off[i]:off[i + 1]]) against the index's targets ->
    {"profile": (m_q, bins) uint32, cell [i, b] the targets of query i's class at a weighted distance d with
    ceil(d / step) == b (not cumulative), "stats": dict over CDR3_PROFILE_STATS}."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    o, t = _node_arrays(off, text)
    m = len(cls)
    if len(o) != m + 1:
        raise ValueError("cdr3_profile_weighted: one class per query, m + 1 offsets")
    step, bins = _u32(step, "step"), _u32(bins, "bins")
    profile = np.empty(max(m * min(bins, CDR3_PROFILE_MAX_BINS), 1), dtype=np.uint32)
    st = Cdr3ProfileStatsC()
    c = cost.as_c() if cost is not None else None
    check(lib().dcrx_cdr3_profile_weighted(index.handle, m, cls.ctypes.data, o.ctypes.data, t.ctypes.data,
                                           C.addressof(c) if c is not None else None, step, bins, profile.ctypes.data, C.byref(st)))
    return {"profile": profile[:m * bins].reshape(m, bins), "stats": {k: int(getattr(st, k)) for k in CDR3_PROFILE_STATS}}


def cdr3_tally_weighted_work_bytes(m_q: int, text_bytes: int, m_t: int) -> int:
    """dcrx_cdr3_tally_weighted_work_bytes."""
    return int(lib().dcrx_cdr3_tally_weighted_work_bytes(int(m_q), int(text_bytes), int(m_t)))


def cdr3_tally_weighted_device(index: Cdr3Index, m_q: int, d_class, d_off, d_text, text_bytes: int, d_weight, cost: Cdr3Cost, d_radius,
                               d_t_count, d_t_weight, d_q_degree, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_tally_weighted_device: per target of the index the queries of a table in HBM (DeviceBuffers) within the target's
    own radius (d_radius, by rank) and their weight, per query the targets it hits, asynchronous on `stream`."""
    def ptr(b):
        return b.ptr if b is not None else None
    c = cost.as_c() if cost is not None else None      # (alive across the call, which copies it)
    check(lib().dcrx_cdr3_tally_weighted_device(index.handle, int(m_q), ptr(d_class), ptr(d_off), ptr(d_text), int(text_bytes),
                                                ptr(d_weight), C.addressof(c) if c is not None else None, ptr(d_radius), ptr(d_t_count),
                                                ptr(d_t_weight), ptr(d_q_degree), ptr(d_work), int(work_bytes), stream))


def cdr3_tally_weighted(index: Cdr3Index, classes, off, text: bytes, weights, cost: Cdr3Cost, radii) -> dict:
    """dcrx_cdr3_tally_weighted: m_q queries (class, string = text[off[i]:off[i + 1]], weight) against the index's targets, each
    with a radius of its own (radii, by rank: 0 .. 65535 or CDR3_NO_RADIUS) -> {"t_count": per target the queries within its
    radius (uint32), "t_weight": the sum of their weights (uint64), "q_degree": per query the targets it hits (uint32), "stats":
    dict over CDR3_TALLY_STATS}."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    o, t = _node_arrays(off, text)
    m = len(cls)
    if len(o) != m + 1 or len(w) != m:
        raise ValueError("cdr3_tally_weighted: one class and one weight per query, m + 1 offsets")
    rr = np.asarray(radii)
    if rr.size and (rr.min() < 0 or rr.max() >= 1 << 32):
        raise ValueError("cdr3_tally_weighted: a radius does not fit 32 bits")
    r = np.ascontiguousarray(rr, dtype=np.uint32)
    m_t = index.info()["targets"]
    if len(r) != m_t:
        raise ValueError(f"cdr3_tally_weighted: {len(r)} radii for {m_t} targets")
    t_count, t_weight, q_degree = np.empty(max(m_t, 1), np.uint32), np.empty(max(m_t, 1), np.uint64), np.empty(max(m, 1), np.uint32)
    st = Cdr3TallyStatsC()
    c = cost.as_c() if cost is not None else None
    check(lib().dcrx_cdr3_tally_weighted(index.handle, m, cls.ctypes.data, o.ctypes.data, t.ctypes.data, w.ctypes.data,
                                         C.addressof(c) if c is not None else None, r.ctypes.data, t_count.ctypes.data,
                                         t_weight.ctypes.data, q_degree.ctypes.data, C.byref(st)))
    return {"t_count": t_count[:m_t], "t_weight": t_weight[:m_t], "q_degree": q_degree[:m],
            "stats": {k: int(getattr(st, k)) for k in CDR3_TALLY_STATS}}


def format_cdr3_matches_weighted(result: dict, v_idx, j_idx, v_calls, j_calls, off, text: bytes, weights, t_off, t_text: bytes,
                                 db_header: bytes, db_lines, cost: Cdr3Cost) -> bytes:
    """dcrx_format_cdr3_matches_weighted: format_cdr3_matches with the weighted distance, computed on the host, in the distance
    column."""
    return format_cdr3_matches(result, v_idx, j_idx, v_calls, j_calls, off, text, weights, t_off, t_text, db_header, db_lines, cost)


def format_cdr3_matches(result: dict, v_idx, j_idx, v_calls, j_calls, off, text: bytes, weights, t_off, t_text: bytes, db_header: bytes,
                        db_lines, metric="hamming") -> bytes:
    """dcrx_format_cdr3_matches: the `.cdr3_matches.tsv` text of a cdr3_match result — per hit the query's rank, calls, string
    and weight, the target's rank, the distance, and the target's database line db_lines[j] (bytes) under db_header.  (metric a
    Cdr3Cost: dcrx_format_cdr3_matches_weighted.)"""
    vi, ji = (np.ascontiguousarray(a, dtype=np.uint32) if len(a) else np.zeros(1, np.uint32) for a in (v_idx, j_idx))
    w = np.ascontiguousarray(weights, dtype=np.uint64) if len(weights) else np.zeros(1, np.uint64)
    (o, t), (to, tt) = _node_arrays(off, text), _node_arrays(t_off, t_text)
    (vc, vo), (jc, jo) = _calls_blob(v_calls), _calls_blob(j_calls)
    lo = np.zeros(len(db_lines) + 1, dtype=np.uint64)
    if len(db_lines):
        lo[1:] = np.cumsum([len(b) for b in db_lines])
    lt = np.frombuffer(b"".join(db_lines) + b"\0", dtype=np.uint8)
    hdr = np.frombuffer(bytes(db_header) + b"\0", dtype=np.uint8)
    hit_off = np.ascontiguousarray(result["hit_off"], dtype=np.uint64)
    hit = np.ascontiguousarray(result["hit"], dtype=np.uint32) if len(result["hit"]) else np.zeros(1, np.uint32)
    args = [len(o) - 1, hit_off.ctypes.data, hit.ctypes.data, vi.ctypes.data, ji.ctypes.data, len(v_calls), vc.ctypes.data, vo.ctypes.data,
            len(j_calls), jc.ctypes.data, jo.ctypes.data, o.ctypes.data, t.ctypes.data, w.ctypes.data, len(to) - 1, to.ctypes.data,
            tt.ctypes.data, hdr.ctypes.data, len(db_header), lo.ctypes.data, lt.ctypes.data]
    if isinstance(metric, Cdr3Cost):
        c = metric.as_c()
        fmt, args = lib().dcrx_format_cdr3_matches_weighted, args + [C.addressof(c)]
    else:
        fmt, args = lib().dcrx_format_cdr3_matches, args + [cdr3_metric_code(metric)]
    need = check(int(fmt(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(fmt(*args, _bytes_address(out), need)))
    return bytes(out[:need])


# ---- the CDR3 network under the weighted metric: include/dcrx.h "the CDR3 network, weighted" ----

def cdr3net_weighted_work_bytes(m: int, text_bytes: int) -> int:
    """dcrx_cdr3net_weighted_work_bytes."""
    return int(lib().dcrx_cdr3net_weighted_work_bytes(int(m), int(text_bytes)))


def cdr3_neighbours_weighted_device(m: int, d_class, d_off, d_text, text_bytes: int, cost: Cdr3Cost, radius: int, d_degree, d_adj_off,
                                    d_adj, d_adj_dist, adj_cap: int, d_adj_need, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_neighbours_weighted_device: cdr3_neighbours_device under the weighted metric; d_adj_dist (may be None)
    receives the neighbours' distances."""
    def ptr(b):
        return b.ptr if b is not None else None
    c = cost.as_c() if cost is not None else None      # (alive across the call, which copies it)
    check(lib().dcrx_cdr3_neighbours_weighted_device(int(m), ptr(d_class), ptr(d_off), ptr(d_text), int(text_bytes),
                                                     C.addressof(c) if c is not None else None, _radius(radius), ptr(d_degree),
                                                     ptr(d_adj_off), ptr(d_adj), ptr(d_adj_dist), int(adj_cap), ptr(d_adj_need),
                                                     ptr(d_work), int(work_bytes), stream))


def cdr3_network_weighted(classes, aa_off, aa_text: bytes, weights, cost: Cdr3Cost, radius: int, want_edges: bool = False):
    """dcrx_cdr3_network_weighted: cdr3_network under the weighted metric — nodes of one class, both of 1 .. 32 letters A .. Z,
    are linked where their weighted distance under `cost` is at most `radius` -> cdr3_network's (result, statistics), the result
    with "adj_dist" (the distance of every adjacency entry, as the device computed it) when edges are wanted."""
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    off, text = _node_arrays(aa_off, aa_text)
    m = len(cls)
    if len(off) != m + 1 or len(w) != m:
        raise ValueError("cdr3_network_weighted: one class and one weight per node, m + 1 offsets")
    if m >= CDR3NET_MAX_NODES:
        raise ValueError(f"the CDR3 network takes fewer than {CDR3NET_MAX_NODES:,} nodes, not {m:,}")
    deg, of, head, nn = (np.zeros(max(m, 1), np.uint32) for _ in range(4))
    cw = np.zeros(max(m, 1), np.uint64)
    adj_off = np.zeros(m + 1, np.uint64) if want_edges else None
    need = C.c_uint64(0)
    st = Cdr3NetworkStatsC()
    c_cost = cost.as_c() if cost is not None else None
    R = _radius(radius)

    def call(adj, dist, cap):
        return check(int(lib().dcrx_cdr3_network_weighted(
            m, cls.ctypes.data, off.ctypes.data, text.ctypes.data, w.ctypes.data, C.addressof(c_cost) if c_cost is not None else None, R,
            deg.ctypes.data, of.ctypes.data, head.ctypes.data, nn.ctypes.data, cw.ctypes.data, adj_off.ctypes.data if want_edges else None,
            adj.ctypes.data if adj is not None else None, dist.ctypes.data if dist is not None else None, cap, C.byref(need), C.byref(st))))
    c = call(None, None, 0)
    result = {"degree": deg[:m].copy(), "cluster_of": of[:m].copy(), "cluster_head": head[:c].copy(), "cluster_size": nn[:c].copy(),
              "cluster_weight": cw[:c].copy()}
    if want_edges:
        adj, dist = np.zeros(max(1, need.value), np.uint32), np.zeros(max(1, need.value), np.uint32)
        if need.value:
            call(adj, dist, need.value)
        result["adj_off"], result["adj"], result["adj_dist"] = adj_off, adj[:need.value], dist[:need.value]
    return result, {k: int(getattr(st, k)) for k in CDR3_NETWORK_STATS}


def format_cdr3_edges_weighted(aa_off, aa_text: bytes, result: dict, cost: Cdr3Cost) -> bytes:
    """dcrx_format_cdr3_edges_weighted: format_cdr3_edges with the weighted distance, computed on the host, in the distance
    column."""
    off, text = _node_arrays(aa_off, aa_text)
    adj_off = np.ascontiguousarray(result["adj_off"], dtype=np.uint64)
    adj = np.ascontiguousarray(result["adj"], dtype=np.uint32) if len(result["adj"]) else np.zeros(1, np.uint32)
    c = cost.as_c() if cost is not None else None
    args = [len(off) - 1, adj_off.ctypes.data, adj.ctypes.data, off.ctypes.data, text.ctypes.data, C.addressof(c) if c is not None else None]
    need = check(int(lib().dcrx_format_cdr3_edges_weighted(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(lib().dcrx_format_cdr3_edges_weighted(*args, _bytes_address(out), need)))
    return bytes(out[:need])


# ---- overlap (the `overlap` sub-command): include/dcrx.h "overlap" ----

def overlap_set_hash_bits(bits: int):
    """dcrx_overlap_set_hash_bits: the bits of the key hash the grouping sorts by (tests; the result does not depend on it)."""
    check(lib().dcrx_overlap_set_hash_bits(int(bits)))


def overlap(samples, classes, off, text: bytes, weights, n_samples: int, min_samples: int = 2):
    """dcrx_overlap_run on the current device, and everything it exports: m rows (sample, class, string =
    text[off[i]:off[i + 1]], weight) of n_samples samples grouped by (class, string) -> (result, statistics dict over
    OVERLAP_STATS, with "rows_per_sample" beside them).
    result: per plane of OVERLAP_PLANES an (n_samples, n_samples) uint64 array; group_of per row (groups numbered by their
    first row); per public row (n_samples >= min_samples; n_samples descending, weight descending, head ascending) head,
    n_samples and weight, and the rows' cells as CSR: cell_off, cell_sample (ascending in a row), cell_weight."""
    smp = np.ascontiguousarray(samples, dtype=np.uint32)
    cls = np.ascontiguousarray(classes, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    o, t = _node_arrays(off, text)
    m, S = len(smp), int(n_samples)
    if len(cls) != m or len(w) != m or len(o) != m + 1:
        raise ValueError("overlap: one sample, one class and one weight per row, m + 1 offsets")
    err = C.c_int(0)
    h = lib().dcrx_overlap_run(S, m, smp.ctypes.data, cls.ctypes.data, o.ctypes.data, t.ctypes.data, w.ctypes.data, int(min_samples),
                               C.byref(err))
    if not h:
        check(err.value if err.value < 0 else -1)
    try:
        n_pub, n_cells, st = C.c_uint64(0), C.c_uint64(0), OverlapStatsC()
        check(lib().dcrx_overlap_info(h, None, None, C.byref(n_pub), C.byref(n_cells), C.byref(st)))
        P, Q = n_pub.value, n_cells.value
        planes = np.zeros((len(OVERLAP_PLANES), S, S), np.uint64)
        group_of, per_sample = np.zeros(max(m, 1), np.uint32), np.zeros(S, np.uint64)
        head, ns, cs = np.zeros(max(P, 1), np.uint32), np.zeros(max(P, 1), np.uint32), np.zeros(max(Q, 1), np.uint32)
        wt, coff, cw = np.zeros(max(P, 1), np.uint64), np.zeros(P + 1, np.uint64), np.zeros(max(Q, 1), np.uint64)
        check(lib().dcrx_overlap_export(h, planes.ctypes.data, group_of.ctypes.data, per_sample.ctypes.data, head.ctypes.data,
                                        ns.ctypes.data, wt.ctypes.data, coff.ctypes.data, cs.ctypes.data, cw.ctypes.data))
    finally:
        lib().dcrx_overlap_destroy(h)
    result = {name: planes[k] for k, name in enumerate(OVERLAP_PLANES)}
    result.update(group_of=group_of[:m], head=head[:P], n_samples=ns[:P], weight=wt[:P], cell_off=coff, cell_sample=cs[:Q],
                  cell_weight=cw[:Q])
    stats = {k: int(getattr(st, k)) for k in OVERLAP_STATS}
    stats["rows_per_sample"] = [int(x) for x in per_sample]
    return result, stats


def overlap_pairs_device(n_groups: int, d_cell_off, d_cell_sample, d_cell_weight, n_samples: int, d_planes, stream=None):
    """dcrx_overlap_pairs_device: the pair accumulation alone over cells in HBM (DeviceBuffers: n_groups + 1 uint32 offsets,
    uint32 samples and weights), ADDED onto d_planes (len(OVERLAP_PLANES) x S x S uint64), asynchronous on `stream`."""
    check(lib().dcrx_overlap_pairs_device(int(n_groups), d_cell_off.ptr, d_cell_sample.ptr, d_cell_weight.ptr, int(n_samples),
                                          d_planes.ptr, stream))


def format_overlap_public(result: dict, sample_names, v_idx, j_idx, v_calls, j_calls, off, text: bytes) -> bytes:
    """dcrx_format_overlap_public: the `overlap_public.tsv` text of an overlap result — per public row the calls
    v_calls[v_idx[head]] and j_calls[j_idx[head]], the head row's string, n_samples, weight, and per sample its cell's weight
    or 0."""
    vi, ji = (np.ascontiguousarray(a, dtype=np.uint32) if len(a) else np.zeros(1, np.uint32) for a in (v_idx, j_idx))
    o, t = _node_arrays(off, text)
    (vc, vo), (jc, jo) = _calls_blob(v_calls), _calls_blob(j_calls)
    names = [x.encode("utf-8", "surrogateescape") for x in sample_names]      # (file names: whatever the file system holds)
    so = np.zeros(len(names) + 1, dtype=np.uint32)
    so[1:] = np.cumsum([len(b) for b in names])
    sc = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
    P = len(result["head"])
    u32 = [np.ascontiguousarray(result[k], dtype=np.uint32) if len(result[k]) else np.zeros(1, np.uint32)
           for k in ("head", "n_samples", "cell_sample")]
    u64 = [np.ascontiguousarray(result[k], dtype=np.uint64) if len(result[k]) else np.zeros(1, np.uint64)
           for k in ("weight", "cell_off", "cell_weight")]
    args = [P, u32[0].ctypes.data, u32[1].ctypes.data, u64[0].ctypes.data, u64[1].ctypes.data, u32[2].ctypes.data, u64[2].ctypes.data,
            len(sample_names), sc.ctypes.data, so.ctypes.data, len(o) - 1, vi.ctypes.data, ji.ctypes.data, len(v_calls), vc.ctypes.data,
            vo.ctypes.data, len(j_calls), jc.ctypes.data, jo.ctypes.data, o.ctypes.data, t.ctypes.data]
    need = check(int(lib().dcrx_format_overlap_public(*args, None, 0)))
    out = _uninitialised_bytes(max(1, need))
    check(int(lib().dcrx_format_overlap_public(*args, _bytes_address(out), need)))
    return bytes(out[:need])


# ---- downsample and the abundance classes (`overlap --downsample`, `overlap --diversity`): include/dcrx.h "downsample" ----

def downsample(samples, weights, n_samples: int, depths, seed: int) -> dict:
    """dcrx_downsample on the current device: m rows (sample, weight), the sample ids non-decreasing, a depth per sample and
    one 64-bit seed -> {"kept": per row the reads of the subsample, "reads": X_s, "depth_used": min(depth_s, X_s),
    "threshold": T_s}, uint64 arrays."""
    smp = np.ascontiguousarray(samples, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    d = np.ascontiguousarray(depths, dtype=np.uint64)
    m, S = len(smp), int(n_samples)
    if len(w) != m or len(d) != S:
        raise ValueError("downsample: one sample and one weight per row, one depth per sample")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("downsample: the seed is 0 .. 2^64 - 1")
    kept = np.zeros(max(m, 1), np.uint64)
    reads, used, thr = (np.zeros(max(S, 1), np.uint64) for _ in range(3))
    check(lib().dcrx_downsample(S, m, smp.ctypes.data, w.ctypes.data, d.ctypes.data if S else None, int(seed), kept.ctypes.data,
                                reads.ctypes.data, used.ctypes.data, thr.ctypes.data))
    return {"kept": kept[:m], "reads": reads[:S], "depth_used": used[:S], "threshold": thr[:S]}


def downsample_work_bytes(m: int, n_samples: int) -> int:
    """dcrx_downsample_work_bytes: the work space dcrx_downsample_device takes (0: refused)."""
    return int(lib().dcrx_downsample_work_bytes(int(m), int(n_samples)))


def downsample_device(n_samples: int, m: int, d_sample, d_weight, d_depth, seed: int, d_kept, d_reads, d_depth_used, d_threshold,
                      d_work, work_bytes: int, stream=None):
    """dcrx_downsample_device: the subsample over rows in HBM (DeviceBuffers), asynchronous on `stream`; nothing is copied
    back."""
    check(lib().dcrx_downsample_device(int(n_samples), int(m), d_sample.ptr, d_weight.ptr, d_depth.ptr, int(seed), d_kept.ptr,
                                       d_reads.ptr, d_depth_used.ptr, d_threshold.ptr, d_work.ptr, int(work_bytes), stream))


# ---- association (`associate`): include/dcrx.h "association" ----

def assoc_permute(masks, mults, n_samples: int, case_mask: int, rank_table, n_ranks: int, tail_ranks: int, permutations: int,
                  seed: int) -> dict:
    """dcrx_assoc_permute on the current device: F features (presence mask uint64, multiplicity uint32) of n_samples samples, the
    case mask, the (n_samples + 1)^2 rank table (uint16, m-major), and `permutations` relabelings from one 64-bit seed ->
    {"obs_rank": per feature its rank under the case mask (uint32), "labels": the relabelings (uint64), "perm_min": per
    relabeling the smallest rank over the features with a multiplicity (uint32), "tail": per rank below tail_ranks the
    (feature, relabeling) pairs that have it, with multiplicity (uint64), "stats": dict over ASSOC_STATS}."""
    mk = np.asarray(masks)
    ml = np.asarray(mults)
    if mk.ndim != 1 or ml.shape != mk.shape:
        raise ValueError("assoc_permute: one mask and one multiplicity per feature")
    if ml.size and (int(ml.min()) < 0 or int(ml.max()) >= 1 << 32):
        raise ValueError("assoc_permute: a multiplicity does not fit 32 bits")
    if not (0 <= int(seed) < 1 << 64 and 0 <= int(case_mask) < 1 << 64):
        raise ValueError("assoc_permute: the seed and the case mask are 0 .. 2^64 - 1")
    for name, v in (("n_samples", n_samples), ("n_ranks", n_ranks), ("tail_ranks", tail_ranks), ("permutations", permutations)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"assoc_permute: {name} does not fit 32 bits")
    mk = np.ascontiguousarray(mk, dtype=np.uint64)
    ml = np.ascontiguousarray(ml, dtype=np.uint32)
    table = np.ascontiguousarray(np.asarray(rank_table).reshape(-1), dtype=np.uint16)
    N, F, P, T = int(n_samples), len(mk), int(permutations), int(tail_ranks)
    if 2 <= N <= ASSOC_MAX_SAMPLES and len(table) != (N + 1) * (N + 1):
        raise ValueError(f"assoc_permute: the rank table holds {len(table)} cells, not (n_samples + 1)^2 = {(N + 1) * (N + 1)}")
    big = P > ASSOC_MAX_PERMUTATIONS or T > (ASSOC_MAX_SAMPLES + 1) ** 2      # (refused in there: nothing that large is made here)
    obs = np.empty(max(F, 1), np.uint32)
    labels, least = np.empty(1 if big else max(P, 1), np.uint64), np.empty(1 if big else max(P, 1), np.uint32)
    tail = np.empty(1 if big else max(T, 1), np.uint64)
    st = AssocStatsC()
    check(lib().dcrx_assoc_permute(N, int(case_mask), F, mk.ctypes.data, ml.ctypes.data, table.ctypes.data, int(n_ranks), T, P, int(seed),
                                   obs.ctypes.data, labels.ctypes.data, least.ctypes.data, tail.ctypes.data, C.byref(st)))
    return {"obs_rank": obs[:F], "labels": labels[:P], "perm_min": least[:P], "tail": tail[:T],
            "stats": {k: int(getattr(st, k)) for k in ASSOC_STATS}}


def assoc_permute_device(n_samples: int, case_mask: int, n_features: int, d_mask, d_mult, d_rank, n_ranks: int, tail_ranks: int,
                         permutations: int, seed: int, d_obs_rank, d_labels, d_perm_min, d_tail, stream=None):
    """dcrx_assoc_permute_device: the permutation null over arrays in HBM (DeviceBuffers; None where an array is empty),
    asynchronous on `stream`; nothing is copied back.  The entry takes no work space."""
    def ptr(b):
        return b.ptr if b is not None else None
    check(lib().dcrx_assoc_permute_device(int(n_samples), int(case_mask), int(n_features), ptr(d_mask), ptr(d_mult), ptr(d_rank),
                                          int(n_ranks), int(tail_ranks), int(permutations), int(seed), ptr(d_obs_rank), ptr(d_labels),
                                          ptr(d_perm_min), ptr(d_tail), stream))


def assoc_case_words(case_words, n_samples: int) -> np.ndarray:
    """The case mask of "association, wide" as ceil(n_samples / 64) uint64 words (at least one): from an array of words or from
    one Python integer (bit s: sample s)."""
    W = max(1, (int(n_samples) + 63) // 64) if 0 <= int(n_samples) <= ASSOC_WIDE_MAX_SAMPLES else 1
    if isinstance(case_words, int):
        if case_words < 0 or case_words >> (64 * W):
            raise ValueError(f"assoc_permute_wide: the case mask does not fit {W} words")
        case_words = [(case_words >> (64 * w)) & ((1 << 64) - 1) for w in range(W)]
    words = np.ascontiguousarray(case_words, dtype=np.uint64).reshape(-1)
    if len(words) != W:
        raise ValueError(f"assoc_permute_wide: the case mask holds {len(words)} words, not ceil(n_samples / 64) = {W}")
    return words


def assoc_permute_wide(masks, mults, n_samples: int, case_words, rank_table, n_ranks: int, tail_ranks: int, permutations: int,
                       seed: int) -> dict:
    """dcrx_assoc_permute_wide on the current device: F features of W = ceil(n_samples / 64) words each (masks[F, W] uint64,
    sample s is bit s & 63 of word s >> 6; multiplicity uint32), the case mask as W words (or one Python integer), the
    (n_samples + 1)^2 rank table (uint32, m-major), and `permutations` relabelings from one 64-bit seed -> {"obs_rank": [F]
    uint32, "labels": [P, W] uint64, "perm_min": [P] uint32, "tail": [tail_ranks] uint64, "stats": dict over ASSOC_STATS}."""
    for name, v in (("n_samples", n_samples), ("n_ranks", n_ranks), ("tail_ranks", tail_ranks), ("permutations", permutations)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"assoc_permute_wide: {name} does not fit 32 bits")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("assoc_permute_wide: the seed is 0 .. 2^64 - 1")
    N, P, T = int(n_samples), int(permutations), int(tail_ranks)
    cases = assoc_case_words(case_words, N)
    W = len(cases)
    mk = np.asarray(masks)
    ml = np.asarray(mults)
    if mk.ndim == 1 and W == 1:
        mk = mk.reshape(-1, 1)
    if mk.ndim != 2 or mk.shape[1] != W or ml.shape != (mk.shape[0],):
        raise ValueError(f"assoc_permute_wide: masks are [F, {W}] with one multiplicity per feature")
    if ml.size and (int(ml.min()) < 0 or int(ml.max()) >= 1 << 32):
        raise ValueError("assoc_permute_wide: a multiplicity does not fit 32 bits")
    mk = np.ascontiguousarray(mk, dtype=np.uint64)
    ml = np.ascontiguousarray(ml, dtype=np.uint32)
    table = np.ascontiguousarray(np.asarray(rank_table).reshape(-1), dtype=np.uint32)
    F = len(mk)
    if 2 <= N <= ASSOC_WIDE_MAX_SAMPLES and len(table) != (N + 1) * (N + 1):
        raise ValueError(f"assoc_permute_wide: the rank table holds {len(table)} cells, not (n_samples + 1)^2 = {(N + 1) * (N + 1)}")
    big = P > ASSOC_MAX_PERMUTATIONS or T > (ASSOC_WIDE_MAX_SAMPLES + 1) ** 2      # (refused in there: nothing that large is made here)
    obs = np.empty(max(F, 1), np.uint32)
    labels, least = np.empty((1 if big else max(P, 1), W), np.uint64), np.empty(1 if big else max(P, 1), np.uint32)
    tail = np.empty(1 if big else max(T, 1), np.uint64)
    st = AssocStatsC()
    check(lib().dcrx_assoc_permute_wide(N, cases.ctypes.data, F, mk.ctypes.data, ml.ctypes.data, table.ctypes.data, int(n_ranks), T, P,
                                        int(seed), obs.ctypes.data, labels.ctypes.data, least.ctypes.data, tail.ctypes.data, C.byref(st)))
    return {"obs_rank": obs[:F], "labels": labels[:P], "perm_min": least[:P], "tail": tail[:T],
            "stats": {k: int(getattr(st, k)) for k in ASSOC_STATS}}


def assoc_permute_wide_device(n_samples: int, case_words, n_features: int, d_mask, d_mult, d_rank, n_ranks: int, tail_ranks: int,
                              permutations: int, seed: int, d_obs_rank, d_labels, d_perm_min, d_tail, stream=None):
    """dcrx_assoc_permute_wide_device: the wide permutation null over arrays in HBM (DeviceBuffers; None where an array is empty)
    — the case mask alone is host memory, W words or one Python integer (None: a null pointer) —, asynchronous on `stream`;
    nothing is copied back.  The entry takes no work space."""
    def ptr(b):
        return b.ptr if b is not None else None
    cases = assoc_case_words(case_words, n_samples) if case_words is not None else None
    check(lib().dcrx_assoc_permute_wide_device(int(n_samples), cases.ctypes.data if cases is not None else None, int(n_features),
                                               ptr(d_mask), ptr(d_mult), ptr(d_rank), int(n_ranks), int(tail_ranks), int(permutations),
                                               int(seed), ptr(d_obs_rank), ptr(d_labels), ptr(d_perm_min), ptr(d_tail), stream))


def assoc_alternative(alternative) -> int:
    """The alternative of "association, rank-sum" as its number: a name of ASSOC_RANKSUM_ALTERNATIVES, or the number itself."""
    if isinstance(alternative, str):
        if alternative not in ASSOC_RANKSUM_ALTERNATIVES:
            raise ValueError(f"assoc_ranksum: the alternative is greater, less or two-sided, not {alternative}")
        return ASSOC_RANKSUM_ALTERNATIVES.index(alternative)
    if not 0 <= int(alternative) < 1 << 32:
        raise ValueError("assoc_ranksum: the alternative does not fit 32 bits")
    return int(alternative)


def assoc_ranksum(planes, offsets, scales, mults, n_samples: int, case_mask: int, alternative, edges, permutations: int, seed: int) -> dict:
    """dcrx_assoc_ranksum on the current device: F features of n_samples samples, each seven bit planes of its scores (planes[F, 7]
    uint64: bit b of sample s's score is bit s of planes[f, b]), an offset, a scale and a multiplicity (uint32), the case mask,
    the alternative (a name or 0 .. 2), the strictly ascending edges of the tail (uint32, at most 1024) and `permutations`
    relabelings from one 64-bit seed -> {"obs_score": per feature its score under the case mask (uint32), "labels": the
    relabelings (uint64), "perm_max": per relabeling the largest score over the features with a multiplicity (uint32), "exceed":
    per feature the relabelings that score at least what the case mask does (uint32), "tail": per edge the (feature, relabeling)
    pairs from it up to the next, with multiplicity (uint64), "stats": dict over ASSOC_RANKSUM_STATS}."""
    pl = np.asarray(planes)
    if pl.ndim != 2 or pl.shape[1] != ASSOC_RANKSUM_PLANES:
        raise ValueError(f"assoc_ranksum: planes are [F, {ASSOC_RANKSUM_PLANES}]")
    F = pl.shape[0]
    per_feature = []
    for name, v in (("offset", offsets), ("scale", scales), ("multiplicity", mults)):
        a = np.asarray(v)
        if a.shape != (F,):
            raise ValueError(f"assoc_ranksum: one {name} per feature")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 32):
            raise ValueError(f"assoc_ranksum: a {name} does not fit 32 bits")
        per_feature.append(np.ascontiguousarray(a, dtype=np.uint32))
    ed = np.asarray(edges)
    if ed.ndim != 1 or (ed.size and (int(ed.min()) < 0 or int(ed.max()) >= 1 << 32)):
        raise ValueError("assoc_ranksum: the edges are one array of 32-bit values")
    if not (0 <= int(seed) < 1 << 64 and 0 <= int(case_mask) < 1 << 64):
        raise ValueError("assoc_ranksum: the seed and the case mask are 0 .. 2^64 - 1")
    for name, v in (("n_samples", n_samples), ("permutations", permutations)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"assoc_ranksum: {name} does not fit 32 bits")
    alt = assoc_alternative(alternative)
    pl = np.ascontiguousarray(pl, dtype=np.uint64)
    ed = np.ascontiguousarray(ed, dtype=np.uint32)
    off, sc, ml = per_feature
    N, P, E = int(n_samples), int(permutations), len(ed)
    big = P > ASSOC_MAX_PERMUTATIONS      # (refused in there: nothing that large is made here)
    obs, exceed = np.empty(max(F, 1), np.uint32), np.empty(max(F, 1), np.uint32)
    labels, most = np.empty(1 if big else max(P, 1), np.uint64), np.empty(1 if big else max(P, 1), np.uint32)
    tail = np.empty(max(E, 1), np.uint64)
    st = AssocRanksumStatsC()
    check(lib().dcrx_assoc_ranksum(N, int(case_mask), alt, F, pl.ctypes.data, off.ctypes.data, sc.ctypes.data, ml.ctypes.data, E, ed.ctypes.data,
                                   P, int(seed), obs.ctypes.data, labels.ctypes.data, most.ctypes.data, exceed.ctypes.data, tail.ctypes.data,
                                   C.byref(st)))
    return {"obs_score": obs[:F], "labels": labels[:P], "perm_max": most[:P], "exceed": exceed[:F], "tail": tail[:E],
            "stats": {k: int(getattr(st, k)) for k in ASSOC_RANKSUM_STATS}}


def assoc_ranksum_device(n_samples: int, case_mask: int, alternative, n_features: int, d_plane, d_offset, d_scale, d_mult, n_edges: int,
                         d_edges, permutations: int, seed: int, d_obs_score, d_labels, d_perm_max, d_exceed, d_tail, stream=None):
    """dcrx_assoc_ranksum_device: the rank-sum null over arrays in HBM (DeviceBuffers; None where an array is empty), asynchronous
    on `stream`; nothing is copied back.  The entry takes no work space."""
    def ptr(b):
        return b.ptr if b is not None else None
    check(lib().dcrx_assoc_ranksum_device(int(n_samples), int(case_mask), assoc_alternative(alternative), int(n_features), ptr(d_plane),
                                          ptr(d_offset), ptr(d_scale), ptr(d_mult), int(n_edges), ptr(d_edges), int(permutations), int(seed),
                                          ptr(d_obs_score), ptr(d_labels), ptr(d_perm_max), ptr(d_exceed), ptr(d_tail), stream))


def abundance_classes(samples, groups, weights, n_samples: int) -> dict:
    """dcrx_abundance_classes on the current device: n items (sample, group, weight) add into cells (sample, group); per
    sample the distinct cell weights ascending with the number of cells of each, as CSR -> {"class_off": n_samples + 1
    offsets, "class_count": the weights, "class_mult": the cells}.  A cell of weight 0 is in no class."""
    smp = np.ascontiguousarray(samples, dtype=np.uint32)
    grp = np.ascontiguousarray(groups, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    n, S = len(smp), int(n_samples)
    if len(grp) != n or len(w) != n:
        raise ValueError("abundance_classes: one sample, one group and one weight per item")
    off = np.zeros(max(S, 0) + 1, np.uint64)
    count, mult = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64)
    k = check(int(lib().dcrx_abundance_classes(S, n, smp.ctypes.data, grp.ctypes.data, w.ctypes.data, off.ctypes.data, count.ctypes.data,
                                               mult.ctypes.data)))
    return {"class_off": off, "class_count": count[:k].copy(), "class_mult": mult[:k].copy()}


# ---- motifs (`motifs`): include/dcrx.h "motifs" ----

def cdr3_motif_k_mask(ks) -> int:
    """The k_mask of K (an iterable of 2, 3, 4)."""
    ks = [int(k) for k in ks]
    if not ks or any(k not in CDR3_MOTIF_KS for k in ks):
        raise ValueError("motifs: K is a non-empty subset of 2, 3, 4")
    return sum(1 << k for k in set(ks))


def cdr3_motif_text(k: int, code: int) -> str:
    """The letters of the motif (k, code)."""
    return "".join(chr(65 + code // 26 ** (k - 1 - i) % 26) for i in range(k))


def cdr3_motifs_work_bytes(n: int, m: int, resamples: int) -> int:
    """dcrx_cdr3_motifs_work_bytes: the work space dcrx_cdr3_motifs_device takes (0: refused)."""
    return int(lib().dcrx_cdr3_motifs_work_bytes(int(n), int(m), int(resamples)))


def cdr3_motifs(s_off, s_text: bytes, b_off, b_text: bytes, ks=CDR3_MOTIF_KS, trim=(3, 3), min_count: int = 3, resamples: int = 1000,
                seed: int = 1, cap: int | None = None) -> dict:
    """dcrx_cdr3_motifs on the current device: n sample units and m background units (offsets into one text each) -> the
    reported motifs in motif order: {"k", "code", "cs", "cb", "ge", "max" (uint32), "sum" (uint64): min(need, cap) rows each,
    "need": the reported motifs, "stats": CDR3_MOTIF_STATS}.  cap None: as many rows as are needed (a second call where the
    first one's guess fell short)."""
    so, bo = np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(b_off, dtype=np.uint64)
    if len(so) < 1 or len(bo) < 1:
        raise ValueError("motifs: count + 1 offsets per side")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("motifs: the seed is 0 .. 2^64 - 1")
    n, m = len(so) - 1, len(bo) - 1
    mask = cdr3_motif_k_mask(ks)
    st, s_buf, b_buf = Cdr3MotifStatsC(), _buf(s_text), _buf(b_text)
    rows = min(n * 90, 475228) if cap is None else int(cap)
    while True:
        out = {name: np.zeros(max(rows, 1), dt) for name, dt in CDR3_MOTIF_OUTPUTS}
        need = np.zeros(1, np.uint64)
        check(lib().dcrx_cdr3_motifs(n, so.ctypes.data, s_buf.ctypes.data, m, bo.ctypes.data, b_buf.ctypes.data, mask, int(trim[0]), int(trim[1]), int(min_count),
                                     int(resamples), int(seed), rows, *(out[name].ctypes.data for name, _ in CDR3_MOTIF_OUTPUTS[:5]),
                                     out["sum"].ctypes.data, out["max"].ctypes.data, need.ctypes.data, C.byref(st)))
        if cap is not None or int(need[0]) <= rows:
            break
        rows = int(need[0])
    got = min(int(need[0]), rows)
    result = {name: out[name][:got].copy() for name, _ in CDR3_MOTIF_OUTPUTS}
    result["need"] = int(need[0])
    result["stats"] = {k: int(getattr(st, k)) for k in CDR3_MOTIF_STATS}
    return result


def cdr3_motifs_device(n: int, d_s_off, d_s_text, m: int, d_b_off, d_b_text, ks, trim, min_count: int, resamples: int, seed: int,
                       cap: int, d_k, d_code, d_cs, d_cb, d_ge, d_sum, d_max, d_need, d_stats, d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_motifs_device: the primitive over units in HBM (DeviceBuffers), asynchronous on `stream`; nothing is copied
    back."""
    check(lib().dcrx_cdr3_motifs_device(int(n), d_s_off.ptr, d_s_text.ptr, int(m), d_b_off.ptr, d_b_text.ptr, cdr3_motif_k_mask(ks),
                                        int(trim[0]), int(trim[1]), int(min_count), int(resamples), int(seed), int(cap), d_k.ptr,
                                        d_code.ptr, d_cs.ptr, d_cb.ptr, d_ge.ptr, d_sum.ptr, d_max.ptr, d_need.ptr, d_stats.ptr,
                                        d_work.ptr, int(work_bytes), stream))


# ---- motif groups (`motifs --groups`): include/dcrx.h "motif groups" ----

def _selected_arrays(sel_k, sel_code):
    k, code = np.ascontiguousarray(sel_k, dtype=np.uint32), np.ascontiguousarray(sel_code, dtype=np.uint32)
    if k.ndim != 1 or k.shape != code.shape:
        raise ValueError("motif groups: one k and one code per selected motif")
    return k, code


def _ptr(a):
    return a.ctypes.data if len(a) else None


def cdr3_motif_members_work_bytes(n: int, cap: int) -> int:
    """dcrx_cdr3_motif_members_work_bytes: the work space dcrx_cdr3_motif_members_device takes (0: refused)."""
    return int(lib().dcrx_cdr3_motif_members_work_bytes(int(n), int(cap)))


def cdr3_groups_work_bytes(n: int, S: int) -> int:
    """dcrx_cdr3_groups_work_bytes: the work space dcrx_cdr3_groups_device takes (0: refused)."""
    return int(lib().dcrx_cdr3_groups_work_bytes(int(n), int(S)))


def cdr3_motif_members_device(n: int, d_off, d_text, ks, trim, S: int, d_sel_k, d_sel_code, cap: int, d_n_motifs, d_mem_off, d_mem, d_need,
                              d_work, work_bytes: int, stream=None):
    """dcrx_cdr3_motif_members_device: the members primitive over units in HBM (DeviceBuffers), asynchronous on `stream`;
    nothing is copied back.  d_mem None with cap 0: a counting call."""
    opt = lambda b: b.ptr if b is not None else None
    check(lib().dcrx_cdr3_motif_members_device(int(n), d_off.ptr, opt(d_text), cdr3_motif_k_mask(ks), int(trim[0]), int(trim[1]), int(S),
                                               opt(d_sel_k), opt(d_sel_code), int(cap), d_n_motifs.ptr, d_mem_off.ptr, opt(d_mem), d_need.ptr,
                                               d_work.ptr, int(work_bytes), stream))


def cdr3_groups_device(n: int, d_weight, d_adj_off, d_adj, adj_entries: int, S: int, d_mem_off, d_mem, mem_entries: int, d_group_of, d_head,
                       d_units, d_weight_out, d_groups, d_work, work_bytes: int, stream=None) -> int:
    """dcrx_cdr3_groups_device: the groups primitive over an adjacency and member rows in HBM (DeviceBuffers), on `stream`
    (it waits for the stream once per round); nothing is copied back.  Returns the number of rounds."""
    opt = lambda b: b.ptr if b is not None else None
    rounds = C.c_uint32(0)
    check(lib().dcrx_cdr3_groups_device(int(n), d_weight.ptr, d_adj_off.ptr, opt(d_adj), int(adj_entries), int(S), opt(d_mem_off), opt(d_mem),
                                        int(mem_entries), d_group_of.ptr, d_head.ptr, d_units.ptr, d_weight_out.ptr, d_groups.ptr,
                                        C.byref(rounds), d_work.ptr, int(work_bytes), stream))
    return int(rounds.value)


def cdr3_motif_groups(off, text: bytes, weights, ks, trim, sel_k, sel_code, distance: int = 1, mem_cap: int | None = None) -> dict:
    """dcrx_cdr3_motif_groups on the current device: n units (offsets into one text) with a weight each, the selected motifs
    (k, code) in motif order and the global distance (0: none) -> {"group_of", "n_motifs", "degree" per unit; "head", "units",
    "weight" per group; "mem_off" (S + 1) and "mem": the members of every selected motif, rows laid end to end; "need": their
    number; "stats": CDR3_MOTIF_GROUP_STATS}.  mem_cap None: the members whole (a second call where the first one's guess
    fell short); otherwise "mem" is empty unless they fit mem_cap."""
    o = np.ascontiguousarray(off, dtype=np.uint64)
    if len(o) < 1:
        raise ValueError("motif groups: count + 1 offsets")
    n = len(o) - 1
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    if len(w) != n:
        raise ValueError("motif groups: one weight per unit")
    k, code = _selected_arrays(sel_k, sel_code)
    S = len(k)
    mask, buf, st = cdr3_motif_k_mask(ks), _buf(text), Cdr3MotifGroupStatsC()
    rows = min(n * min(S, 90), 1 << 22) if mem_cap is None else int(mem_cap)
    while True:
        group_of, n_motifs, degree, head, units = (np.zeros(max(n, 1), np.uint32) for _ in range(5))
        weight_out, mem_off, mem = np.zeros(max(n, 1), np.uint64), np.zeros(S + 1, np.uint64), np.zeros(max(rows, 1), np.uint32)
        need = C.c_uint64(0)
        check(lib().dcrx_cdr3_motif_groups(n, o.ctypes.data, buf.ctypes.data, w.ctypes.data, mask, int(trim[0]), int(trim[1]), S, _ptr(k),
                                           _ptr(code), int(distance), group_of.ctypes.data, n_motifs.ctypes.data, degree.ctypes.data,
                                           head.ctypes.data, units.ctypes.data, weight_out.ctypes.data, mem_off.ctypes.data,
                                           mem.ctypes.data if rows else None, rows, C.byref(need), C.byref(st)))
        if mem_cap is not None or need.value <= rows:
            break
        rows = int(need.value)
    g = int(st.groups)
    return {"group_of": group_of[:n].copy(), "n_motifs": n_motifs[:n].copy(), "degree": degree[:n].copy(), "head": head[:g].copy(),
            "units": units[:g].copy(), "weight": weight_out[:g].copy(), "mem_off": mem_off,
            "mem": mem[:need.value].copy() if need.value <= rows else mem[:0].copy(), "need": int(need.value),
            "stats": {f: int(getattr(st, f)) for f in CDR3_MOTIF_GROUP_STATS}}


def cdr3_motif_members(off, text: bytes, ks, trim, sel_k, sel_code, cap: int | None = None, stream=None) -> dict:
    """dcrx_cdr3_motif_members_device over host arrays (uploaded here, copied back here): {"n_motifs" per unit, "mem_off"
    (S + 1), "mem": min(need, cap) members, "need"}.  cap None: a counting call, then exactly `need`; cap 0: the counting call
    alone."""
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(o) - 1
    k, code = _selected_arrays(sel_k, sel_code)
    S = len(k)
    d_off, d_text = DeviceBuffer.from_host(o), DeviceBuffer.from_host(_buf(text))
    d_k, d_code = (DeviceBuffer.from_host(a) if S else None for a in (k, code))
    d_nm, d_mo, d_need = DeviceBuffer(4 * max(n, 1)), DeviceBuffer(8 * (S + 1)), DeviceBuffer(16)

    def call(rows):
        bytes_ = cdr3_motif_members_work_bytes(n, rows)
        if not bytes_:
            raise ValueError("motif members: 2^30 units or more, or cap + n is 2^31 or more")
        d_work, d_mem = DeviceBuffer(bytes_), DeviceBuffer(4 * rows) if rows else None
        cdr3_motif_members_device(n, d_off, d_text, ks, trim, S, d_k, d_code, rows, d_nm, d_mo, d_mem, d_need, d_work, bytes_, stream)
        if stream is not None:
            check(lib().dcrx_stream_synchronize(stream))
        else:
            synchronize()
        return d_mem
    d_mem = call(0 if cap is None else int(cap))
    need = int(d_need.to_host(np.uint64, 1)[0])
    rows = need if cap is None else int(cap)
    if cap is None and need:
        d_mem = call(need)
    got = min(need, rows)
    return {"n_motifs": d_nm.to_host(np.uint32, n), "mem_off": d_mo.to_host(np.uint64, S + 1),
            "mem": d_mem.to_host(np.uint32, got) if got else np.zeros(0, np.uint32), "need": need}


def merge_parents_device(tables: "Tables", n: int, d_v, d_j, d_vdel, d_jdel, d_count, d_ins_off, d_ins_text, text_bytes: int,
                         distance: int, ratio: int, d_parent, d_reach, d_work, work_bytes: int, stream=None):
    """dcrx_merge_parents_device: parent(c) of every entry of a counted table in HBM (DeviceBuffers), asynchronous on `stream`."""
    check(lib().dcrx_merge_parents_device(tables.handle, int(n), d_v.ptr, d_j.ptr, d_vdel.ptr, d_jdel.ptr, d_count.ptr, d_ins_off.ptr,
                                          d_ins_text.ptr if d_ins_text is not None else None, int(text_bytes), int(distance),
                                          int(ratio), d_parent.ptr, d_reach.ptr if d_reach is not None else None, d_work.ptr,
                                          int(work_bytes), stream))


def _index_arg(index, n):
    if index is None:
        return None, None
    idx = np.ascontiguousarray(index, dtype=np.uint32)
    if idx.shape != (n,):
        raise ValueError("index: one uint32 entry per read of the batch")
    return idx, idx.ctypes.data


def decombine_count(tables: Tables, batch: PackedBatch, counts: DcrCounts, first_index: int = 0, index=None,
                    orientation="reverse", allow_ns=False, lenthreshold=130, flags=0) -> np.ndarray:
    """dcrx_decombine_count: the batch decombined and its DCRs added into `counts`, read r as ordinal first_index + r (or
    first_index + index[r]).  Returns the counters (uint64[32]); no records come back."""
    cfg = make_cfg(orientation, allow_ns, lenthreshold, flags)
    return _host_call([tables], batch, cfg, counts_list=[counts], first_index=first_index, index=index, chains=False)[0]


def decombine_chains_count(tables_list, batch: PackedBatch, counts_list, first_index: int = 0, index=None,
                           orientation="reverse", allow_ns=False, lenthreshold=130, flags=0) -> list:
    """dcrx_decombine_chains_count: one upload of the batch, chain c's DCRs added into counts_list[c].  Returns the counters
    per chain; each equals what decombine_count() gives for that chain alone."""
    tables_list, counts_list = list(tables_list), list(counts_list)
    if len(tables_list) != len(counts_list):
        raise ValueError("one DcrCounts per chain")
    cfg = make_cfg(orientation, allow_ns, lenthreshold, flags)
    return _host_call(tables_list, batch, cfg, counts_list=counts_list, first_index=first_index, index=index)


def count_dcrs(tables_list, batch: PackedBatch, counts_list, first_index: int = 0, index=None, orientation="reverse",
               allow_ns=False, lenthreshold=130) -> list:
    """The barcode-free stage's one call per batch: decombine the batch for every chain and add its DCRs into that chain's
    DcrCounts (dcrx_decombine_chains_count: one upload, whatever the number of chains).  Returns the counters per chain."""
    return decombine_chains_count(tables_list, batch, counts_list, first_index, index, orientation, allow_ns, lenthreshold)


def count_device(counts: DcrCounts, d_records: "DeviceBuffer", batch: "DeviceBatch", first_index: int = 0,
                 d_index: "DeviceBuffer | None" = None, stream=None):
    """dcrx_count_device: the count step over records already in HBM, asynchronous on `stream`."""
    b = batch.as_c()
    check(lib().dcrx_count_device(counts.handle, d_records.ptr, C.byref(b), int(first_index),
                                  d_index.ptr if d_index is not None else None, stream))


def synth_cfg(seed: int, read_len: int = 150, p_rearranged: float = 0.45, sub_rate: float = 0.005,
              n_rate: float = 0.0005) -> SynthCfgC:
    return SynthCfgC(int(seed), int(read_len), float(p_rearranged), float(sub_rate), float(n_rate))


def synth_reads_host(tables: Tables, cfg: SynthCfgC, first: int, n: int, stride: int | None = None, pinned: bool = False) -> PackedBatch:
    """Seeded synthetic reads [first, first+n) generated by the library on the host."""
    if stride is None:
        stride = stride_for(cfg.read_len)
    packed = pinned_empty((n, stride), np.uint8) if pinned else np.zeros((n, stride), dtype=np.uint8)
    check(lib().dcrx_synth_reads_host(tables.handle, C.byref(cfg), first, n, stride,
                                      packed.ctypes.data if n else None))
    er, ep, ec = synth_exceptions_host(tables, cfg, first, n)
    return PackedBatch(packed, stride, cfg.read_len, None, er, ep, ec)


def synth_exceptions_host(tables: Tables, cfg: SynthCfgC, first: int, n: int):
    cap = max(16, int(n * cfg.n_rate * 2) + 64)
    while True:
        er = np.zeros(cap, dtype=np.uint32)
        ep = np.zeros(cap, dtype=np.uint16)
        ec = np.zeros(cap, dtype=np.uint8)
        got = int(lib().dcrx_synth_exceptions_host(tables.handle, C.byref(cfg), first, n, er.ctypes.data,
                                                   ep.ctypes.data, ec.ctypes.data, cap))
        check(got)
        if got <= cap:
            return er[:got].copy(), ep[:got].copy(), ec[:got].copy()
        cap = got


def device_count() -> int:
    return int(lib().dcrx_device_count())


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(lib().dcrx_device_name(buf, 256))
    return buf.value.decode()


# ---- device-resident path (no torch needed: the library owns the HIP calls) ----

class DeviceBuffer:
    """A hipMalloc'd buffer owned through the C ABI."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().dcrx_malloc_device(C.byref(p), int(nbytes)))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    @classmethod
    def from_host(cls, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        buf = cls(max(arr.nbytes, 16))
        if arr.nbytes:
            check(lib().dcrx_memcpy_h2d(buf.ptr, arr.ctypes.data, arr.nbytes))
        return buf

    def to_host(self, dtype, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=dtype)
        if out.nbytes:
            check(lib().dcrx_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().dcrx_free_device(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBatch:
    """Packed reads resident in HBM (the buffers dcrx_decombine_device reads)."""

    def __init__(self, n_reads: int, stride: int, read_len: int, packed: DeviceBuffer,
                 lens: DeviceBuffer | None = None, exc=None):
        self.n_reads, self.stride, self.read_len = int(n_reads), int(stride), int(read_len)
        self.packed, self.lens = packed, lens
        self.exc = exc  # (n_exc, DeviceBuffer read, DeviceBuffer pos, DeviceBuffer chr) or None

    @classmethod
    def from_host(cls, b: PackedBatch) -> "DeviceBatch":
        exc = None
        if len(b.exc_read):
            exc = (len(b.exc_read), DeviceBuffer.from_host(b.exc_read), DeviceBuffer.from_host(b.exc_pos),
                   DeviceBuffer.from_host(b.exc_chr))
        # 16 spare bytes after the last read (word-pair loads of the final read)
        packed = DeviceBuffer(b.packed.nbytes + 16)
        if b.packed.nbytes:
            check(lib().dcrx_memcpy_h2d(packed.ptr, b.packed.ctypes.data, b.packed.nbytes))
        return cls(b.n_reads, b.stride, b.read_len, packed,
                   DeviceBuffer.from_host(b.lens) if b.lens is not None else None, exc)

    def as_c(self) -> BatchC:
        b = BatchC()
        b.n_reads, b.packed, b.stride, b.read_len = self.n_reads, self.packed.ptr, self.stride, self.read_len
        b.lens = self.lens.ptr if self.lens is not None else None
        if self.exc:
            b.n_exc, b.exc_read, b.exc_pos, b.exc_chr = self.exc[0], self.exc[1].ptr, self.exc[2].ptr, self.exc[3].ptr
        else:
            b.n_exc, b.exc_read, b.exc_pos, b.exc_chr = 0, None, None, None
        return b


def synth_reads_device(tables: Tables, cfg: SynthCfgC, first: int, n: int, stride: int | None = None,
                       stream=None) -> DeviceBatch:
    """Same reads as synth_reads_host, generated in HBM by the library's kernel."""
    if stride is None:
        stride = stride_for(cfg.read_len)
    packed = DeviceBuffer(n * stride + 16)
    check(lib().dcrx_synth_reads_device(tables.handle, C.byref(cfg), first, n, stride, packed.ptr, stream))
    er, ep, ec = synth_exceptions_host(tables, cfg, first, n)
    exc = None
    if len(er):
        exc = (len(er), DeviceBuffer.from_host(er), DeviceBuffer.from_host(ep), DeviceBuffer.from_host(ec))
    return DeviceBatch(n, stride, cfg.read_len, packed, None, exc)


def decombine_device(tables: Tables, batch: DeviceBatch, d_records: DeviceBuffer, d_counters: DeviceBuffer,
                     orientation="reverse", allow_ns=False, lenthreshold=130, flags=0, stream=None):
    """Asynchronous launch on `stream` (None = default); results stay in HBM."""
    cfg = make_cfg(orientation, allow_ns, lenthreshold, flags)
    b = batch.as_c()
    check(lib().dcrx_decombine_device(tables.handle, C.byref(cfg), C.byref(b), d_records.ptr, d_counters.ptr, stream))


def synchronize():
    check(lib().dcrx_synchronize())


class Event:
    def __init__(self, timing: bool = True):
        p = C.c_void_p()
        check((lib().dcrx_event_create if timing else lib().dcrx_event_create_ordering)(C.byref(p)))      # (timing=False: for ordering streams only, cheaper to record)
        self.ptr = p.value

    def record(self, stream=None):
        check(lib().dcrx_event_record(self.ptr, stream))

    def synchronize(self):
        check(lib().dcrx_event_synchronize(self.ptr))

    def elapsed_ms(self, later: "Event") -> float:
        ms = C.c_float()
        check(lib().dcrx_event_elapsed_ms(self.ptr, later.ptr, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if self.ptr:
                lib().dcrx_event_destroy(self.ptr)
        except Exception:
            pass


class Stream:
    """A HIP stream of the caller's own (dcrx_stream_create): a sharded run's side stream for the exchange."""

    def __init__(self):
        p = C.c_void_p()
        check(lib().dcrx_stream_create(C.byref(p)))
        self.ptr = p.value

    def synchronize(self):
        check(lib().dcrx_stream_synchronize(self.ptr))

    def wait_event(self, ev: "Event"):
        check(lib().dcrx_stream_wait_event(self.ptr, ev.ptr))

    def __del__(self):
        try:
            if self.ptr:
                lib().dcrx_stream_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


# ---- multi-GPU: RCCL bound by the library itself (include/dcrx.h, "multi-GPU") ----
COMM_ID_BYTES = 128
COMM_SUM, COMM_MAX = 0, 1


@contextlib.contextmanager
def _c_stdout_to_stderr():
    """RCCL greets on the C library's stdout when a communicator is made (version, host, library path): a process whose stdout
    is a result — bench.py prints ONE JSON line there — sends that to stderr instead (the descriptor itself, around the call)."""
    libc = C.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


class Comm:
    """An RCCL communicator through the C ABI: one process per GPU (`Comm(uid, world, rank)` after dcrx_set_device), the id drawn
    by rank 0 (`Comm.unique_id()`) and carried to the others by the caller — `comm_from_env()` does that for ranks started on one
    node by torch.distributed.run or by bench.py's own spawn.  No torch anywhere."""

    def __init__(self, uid: bytes, world: int, rank: int):
        assert len(uid) == COMM_ID_BYTES
        self._uid = np.frombuffer(uid, dtype=np.uint8).copy()
        h = C.c_void_p()
        with _c_stdout_to_stderr():
            rc = lib().dcrx_comm_create(self._uid.ctypes.data, int(world), int(rank), C.byref(h))
        check(rc)
        self.handle, self.world, self.rank = h.value, int(world), int(rank)

    @staticmethod
    def available() -> bool:
        return bool(lib().dcrx_comm_available())

    @staticmethod
    def unique_id() -> bytes:
        buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
        check(lib().dcrx_comm_unique_id(buf.ctypes.data))
        return buf.tobytes()

    # --- device memory, asynchronous on `stream` (a pointer or None) ---
    def allreduce_u64(self, d_in: int, d_out: int, n: int, op: int = COMM_SUM, stream=None):
        check(lib().dcrx_comm_allreduce_u64(self.handle, d_in, d_out, int(n), op, stream))

    def allreduce_f64(self, d_in: int, d_out: int, n: int, op: int = COMM_MAX, stream=None):
        check(lib().dcrx_comm_allreduce_f64(self.handle, d_in, d_out, int(n), op, stream))

    def allgather(self, d_in: int, d_out: int, bytes_per_rank: int, stream=None):
        check(lib().dcrx_comm_allgather(self.handle, d_in, d_out, int(bytes_per_rank), stream))

    def gather_v(self, d_send: int, send_bytes: int, d_recv=None, recv_bytes=None, root: int = 0, stream=None):
        """Every rank but `root` sends send_bytes from d_send; the root receives recv_bytes[r] into d_recv[r] (one group)."""
        ptrs = sizes = None
        if self.rank == root and self.world > 1:
            ptrs = (C.c_void_p * self.world)(*[int(p) if p else None for p in d_recv])
            sizes = (C.c_uint64 * self.world)(*[int(b) for b in recv_bytes])
        check(lib().dcrx_comm_gather_v(self.handle, d_send, int(send_bytes), ptrs, sizes, int(root), stream))

    def barrier(self, stream=None):
        check(lib().dcrx_comm_barrier(self.handle, stream))

    # --- host memory, synchronous: the control plane of a sharded run ---
    def allgather_host(self, arr: np.ndarray) -> np.ndarray:
        """Every rank's array (same shape and dtype on all ranks), stacked in rank order."""
        a = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + a.shape, dtype=a.dtype)
        check(lib().dcrx_comm_allgather_host(self.handle, a.ctypes.data if a.nbytes else None, out.ctypes.data if out.nbytes else None, a.nbytes))
        return out

    def allreduce_host_u64(self, values, op: int = COMM_SUM) -> np.ndarray:
        a = np.ascontiguousarray(values, dtype=np.uint64).copy()
        check(lib().dcrx_comm_allreduce_host_u64(self.handle, a.ctypes.data if a.size else None, a.size, op))
        return a

    def allgather_bytes(self, blob: bytes) -> list:
        """Every rank's bytes, in rank order (sizes first, then one padded all-gather)."""
        sizes = self.allgather_host(np.array([len(blob)], dtype=np.uint64)).reshape(-1)
        kmax = int(sizes.max()) if sizes.size else 0
        if kmax == 0:
            return [b"" for _ in range(self.world)]
        pad = np.zeros(kmax, dtype=np.uint8)
        pad[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        got = self.allgather_host(pad)
        return [got[r, :int(sizes[r])].tobytes() for r in range(self.world)]

    def allgather_object(self, obj) -> list:
        import pickle
        return [pickle.loads(b) for b in self.allgather_bytes(pickle.dumps(obj))]

    def gather_bytes(self, blob: bytes, dst: int = 0):
        """Every rank's bytes on `dst`, in rank order (a list there, None elsewhere): the sizes (an all-gather), then one exact-size
        transfer per peer from device memory into device memory (dcrx_comm_gather_v), waited for before this returns."""
        sizes = [int(x) for x in self.allgather_host(np.array([len(blob)], dtype=np.uint64)).reshape(-1)]
        if self.world == 1:
            return [blob]
        mine = DeviceBuffer.from_host(np.frombuffer(blob, dtype=np.uint8)) if len(blob) else DeviceBuffer(16)
        recv = None
        if self.rank == dst:
            recv = [DeviceBuffer(max(n, 16)) if r != dst else None for r, n in enumerate(sizes)]
        self.gather_v(mine.ptr, len(blob), [b.ptr if b is not None else None for b in recv] if recv else None, sizes if recv else None, dst, None)
        synchronize()
        if self.rank != dst:
            return None
        return [blob if r == dst else recv[r].to_host(np.uint8, sizes[r]).tobytes() for r in range(self.world)]

    def close(self):
        if getattr(self, "handle", None):
            with _c_stdout_to_stderr():
                lib().dcrx_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_from_env(timeout_s: float = 300.0) -> Comm:
    """The communicator of a rank started with RANK / WORLD_SIZE / LOCAL_RANK / MASTER_PORT in its environment (one node:
    torch.distributed.run, bench.py's spawn).  Rank 0 draws the id and leaves it in a file of the node's temporary directory —
    named for the launcher's port and the launcher's process, which every rank of one launch shares and no other launch does —
    written under another name and renamed, so that a reader never sees half of it; the others wait for the file.  Rank 0
    removes it once every rank has joined (the communicator exists).  DCRX_COMM_ID_FILE overrides the path (a shared file
    system carries the id between nodes the same way)."""
    import tempfile
    import time
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    path = os.environ.get("DCRX_COMM_ID_FILE")
    if not path:
        key = f"{os.environ.get('MASTER_PORT', '0')}_{os.environ.get('TORCHELASTIC_RUN_ID', 'none')}_{os.getppid()}"
        path = os.path.join(tempfile.gettempdir(), f"dcrx_comm_id_{key}")
    if rank == 0:
        uid = Comm.unique_id()
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "wb") as fh:
            fh.write(uid)
        os.replace(tmp, path)
    else:
        t0 = time.time()
        while True:
            try:
                with open(path, "rb") as fh:
                    uid = fh.read()
                if len(uid) == COMM_ID_BYTES:
                    break
            except OSError:
                pass
            if time.time() - t0 > timeout_s:
                raise TimeoutError(f"rank {rank}: no communicator id at {path} after {timeout_s:.0f} s (did rank 0 start?)")
            time.sleep(0.01)
    comm = Comm(uid, world, rank)
    if rank == 0:
        try:
            os.remove(path)
        except OSError:
            pass
    return comm


def compact_hits_bitmap_device(d_records: DeviceBuffer, n_reads: int, d_hits: DeviceBuffer, d_ok_bitmap: DeviceBuffer,
                               d_n_hits: DeviceBuffer, stream=None):
    """Decombined records in input order + a bitmap of which reads they belong to ((n_reads+63)//64 uint64)."""
    check(lib().dcrx_compact_hits_bitmap_device(d_records.ptr, n_reads, d_hits.ptr, d_ok_bitmap.ptr, d_n_hits.ptr, stream))


def pack_tuples8(rec) -> np.ndarray:
    """Host-side twin of dcrx_compact_hits_packed8_device: the status-OK records of `rec` as (k, 2) uint32 tuples in read order."""
    r = rec[rec["status"] == 0]
    w = np.zeros((len(r), 2), dtype=np.uint32)
    jd = r["jdel"].astype(np.uint32)
    w[:, 0] = (r["v"].astype(np.uint32) & 0x7FF) | ((r["j"].astype(np.uint32) & 0x1FF) << 11) | (r["vdel"].astype(np.uint32) << 20) | ((jd & 0xF) << 28)
    w[:, 1] = (jd >> 4) | ((r["v_start"].astype(np.uint32) & 0x1FF) << 4) | ((r["j_end"].astype(np.uint32) & 0x1FF) << 13) | \
              ((r["ins_len"].astype(np.uint32) & 0x1FF) << 22) | ((r["frame"].astype(np.uint32) & 1) << 31)
    return w


def unpack_tuples8(words: np.ndarray, v_jumps) -> np.ndarray:
    """(k, 2) uint32 tuples of dcrx_compact_hits_packed8_device -> RECORD_DTYPE records (status OK).  ins_start, which the
    tuple leaves out, is the base after the end of V: v_start + jump_to_end_v[v] - vdel (decombine.py:283-285, :547, :577)."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 2)
    rec = np.zeros(len(w), dtype=RECORD_DTYPE)
    rec["v"] = w[:, 0] & 0x7FF
    rec["j"] = (w[:, 0] >> 11) & 0x1FF
    rec["vdel"] = (w[:, 0] >> 20) & 0xFF
    rec["jdel"] = ((w[:, 0] >> 28) & 0xF) | ((w[:, 1] & 0xF) << 4)
    rec["v_start"] = (w[:, 1] >> 4) & 0x1FF
    rec["j_end"] = (w[:, 1] >> 13) & 0x1FF
    rec["ins_len"] = (w[:, 1] >> 22) & 0x1FF
    rec["frame"] = (w[:, 1] >> 31) & 1
    jumps = np.asarray(v_jumps, dtype=np.int64)
    rec["ins_start"] = rec["v_start"].astype(np.int64) + jumps[rec["v"].astype(np.int64)] - rec["vdel"].astype(np.int64)
    return rec


class TupleCodec:
    """The narrow tuple of include/dcrx.h (dcrx_tuple_layout) on the host: the layout of a tag set for reads of up to
    max_read_len nt, the host-side twin of dcrx_compact_hits_narrow_device (`pack`) and the receiver's side (`unpack`)."""

    def __init__(self, tables: "Tables", max_read_len: int):
        self.layout = TupleLayoutC()
        check(lib().dcrx_tuple_layout(tables.handle, int(max_read_len), C.byref(self.layout)))
        L = self.layout
        self.bytes, self.bits = int(L.bytes), int(L.bits)
        self.widths = [int(L.w_v), int(L.w_j), int(L.w_vdel), int(L.w_jdel), int(L.w_pos), int(L.w_pos), 1, 1]
        self.v_jumps = np.asarray(tables.v_jumps, dtype=np.int64)
        self.j_jumps = np.asarray(tables.j_jumps, dtype=np.int64)
        self.j_lens = np.asarray(tables.j_lens, dtype=np.int64)
        self.j_short = 2 * int(tables.j_half_split)

    def message_bytes(self, n_reads: int, n_hits: int) -> int:
        return ((n_reads + 63) // 64) * 8 + n_hits * self.bytes

    def pack(self, rec, n_slots: int = None) -> np.ndarray:
        """The message of a batch's records (uint8): bitmap (over n_slots >= len(rec) read slots), low words, high bytes."""
        n_slots = len(rec) if n_slots is None else n_slots
        ok = rec["status"] == 0
        r = rec[ok]
        j = r["j"].astype(np.int64)
        tagpos = r["ins_start"].astype(np.int64) + r["ins_len"].astype(np.int64) - r["jdel"].astype(np.int64) + self.j_jumps[j]
        short_end = ((r["j_end"].astype(np.int64) - tagpos) != self.j_lens[j]).astype(np.uint64)
        fields = [r["v"], r["j"], r["vdel"], r["jdel"], r["v_start"], r["j_end"], short_end, r["frame"] & 1]
        t = np.zeros(len(r), dtype=np.uint64)
        sh = 0
        for f, w in zip(fields, self.widths):
            t |= f.astype(np.uint64) << np.uint64(sh)
            sh += w
        bits = np.zeros(((n_slots + 63) // 64) * 64, dtype=np.uint8)
        bits[:len(rec)] = ok
        bitmap = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
        lo = (t & np.uint64(0xFFFFFFFF)).astype("<u4").view(np.uint8)
        hi = (t >> np.uint64(32)).astype("<u8").view(np.uint8).reshape(-1, 8)[:, :self.bytes - 4].reshape(-1)
        return np.concatenate([bitmap, lo, hi])

    def unpack(self, message, n_reads: int, n_hits: int):
        """(records (status OK), read indices) of a message of n_hits tuples over n_reads reads."""
        m = np.ascontiguousarray(message, dtype=np.uint8)
        bm = ((n_reads + 63) // 64) * 8
        idx = np.nonzero(np.unpackbits(m[:bm], bitorder="little")[:n_reads])[0]
        t = m[bm:bm + 4 * n_hits].view("<u4").astype(np.uint64)
        hb = self.bytes - 4
        if hb:
            hi = np.zeros((n_hits, 8), dtype=np.uint8)
            hi[:, :hb] = m[bm + 4 * n_hits:bm + self.bytes * n_hits].reshape(n_hits, hb)
            t |= hi.view("<u8").reshape(-1) << np.uint64(32)
        vals = []
        sh = 0
        for w in self.widths:
            vals.append(((t >> np.uint64(sh)) & np.uint64((1 << w) - 1)).astype(np.int64))
            sh += w
        v, j, vdel, jdel, v_start, j_end, short_end, frame = vals
        rec = np.zeros(n_hits, dtype=RECORD_DTYPE)
        for name, x in (("v", v), ("j", j), ("vdel", vdel), ("jdel", jdel), ("v_start", v_start), ("j_end", j_end), ("frame", frame)):
            rec[name] = x
        ins_start = v_start + self.v_jumps[v] - vdel
        start_j = j_end - np.where(short_end == 1, self.j_short, self.j_lens[j]) - self.j_jumps[j] + jdel
        rec["ins_start"] = ins_start
        rec["ins_len"] = start_j - ins_start
        return rec, idx


def compact_hits_narrow_device(tables: "Tables", codec: TupleCodec, d_records_ptr: int, n_reads: int, d_message_ptr: int,
                               d_n_hits_ptr: int, stream=None, n_slots: int = None):
    check(lib().dcrx_compact_hits_narrow_device(tables.handle, C.byref(codec.layout), d_records_ptr, n_reads,
                                                n_reads if n_slots is None else n_slots, d_message_ptr, d_n_hits_ptr, stream))


def set_tuple_sink(tables: "Tables", codec, d_message_ptr: int = 0, n_slots: int = 0, d_n_hits_ptr: int = 0):
    """dcrx_set_tuple_sink: the next dcrx_decombine_device calls on `tables` also leave the batch's message; codec None: off."""
    if codec is None:
        check(lib().dcrx_set_tuple_sink(tables.handle, None, None, 0, None))
    else:
        check(lib().dcrx_set_tuple_sink(tables.handle, C.byref(codec.layout), d_message_ptr, n_slots, d_n_hits_ptr))


def unpack_tuples12(words: np.ndarray) -> np.ndarray:
    """(k, 3) uint32 tuples of dcrx_compact_hits_packed_device -> RECORD_DTYPE records (status OK)."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 3)
    rec = np.zeros(len(w), dtype=RECORD_DTYPE)
    rec["v"] = w[:, 0] & 0xFFF
    rec["j"] = (w[:, 0] >> 12) & 0xFFF
    rec["vdel"] = (w[:, 0] >> 24) & 0xFF
    rec["v_start"] = w[:, 1] & 0x1FF
    rec["j_end"] = (w[:, 1] >> 9) & 0x1FF
    rec["ins_start"] = (w[:, 1] >> 18) & 0x1FF
    rec["ins_len"] = w[:, 2] & 0x1FF
    rec["jdel"] = (w[:, 2] >> 9) & 0xFF
    rec["frame"] = (w[:, 2] >> 17) & 1
    return rec


def compact_hits_device(d_records: DeviceBuffer, n_reads: int, first_index: int, d_hits: DeviceBuffer,
                        d_hit_index: DeviceBuffer, d_n_hits: DeviceBuffer, stream=None):
    check(lib().dcrx_compact_hits_device(d_records.ptr, n_reads, first_index, d_hits.ptr, d_hit_index.ptr,
                                         d_n_hits.ptr, stream))
