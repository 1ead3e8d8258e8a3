/*
 * dcrx.h — C ABI of the MI355X-native `decombine` hot path.
 *
 * The reference (innate2adaptive/decombinator, pure Python) has no FFI or plugin
 * interface; its narrowest seam around this path is
 *
 *     decombine.import_tcr_info(inputargs)      src/decombinator/decombine.py:593-746
 *     decombine.dcr(read, inputargs) -> 7-list  src/decombinator/decombine.py:534-585
 *     the per-read driver loop                  src/decombinator/decombine.py:963-1050
 *
 * Each entry point below names the reference code it replaces.  A maintainer
 * binds this library with ctypes (INTEGRATION.md shows the stub); all pointers
 * are plain buffers owned by the caller, the only library-owned object is the
 * opaque dcrx_tables_t handle.
 *
 * Conventions
 *   - every function returns 0 on success or a negative dcrx_error; the text of
 *     the last failure on the calling thread is dcrx_last_error();
 *   - nothing throws, aborts or prints;
 *   - a dcrx_tables_t is not thread-safe: serialise calls that share one, and launch the
 *     asynchronous entry points that share one on ONE stream (the handle owns a workspace
 *     that consecutive launches reuse).  A launch may fork part of its work onto a stream the
 *     handle owns and joins it back before its last kernel: to the caller it is ordered on
 *     the stream it was given, like any other work there;
 *   - "device" pointers are HIP device memory on the current device
 *     (dcrx_set_device), "host" pointers ordinary process memory.
 */
#ifndef DCRX_H
#define DCRX_H

#include <stddef.h>
#include <stdint.h>

#include "dcrx_codes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCRX_ABI_VERSION 5

enum dcrx_error {
  DCRX_OK = 0,
  DCRX_E_INVALID = -1,      /* bad argument */
  DCRX_E_UNSUPPORTED = -2,  /* tag set outside what the device tables can express (see dcrx_tables_create) */
  DCRX_E_NOMEM = -3,
  DCRX_E_HIP = -4,          /* a HIP runtime call failed (no GPU, launch failure, ...) */
  DCRX_E_NOGPU = -5
};

/* ---- tables: replaces import_tcr_info's module globals (decombine.py:593-746) ---- */

/* What get_v_tags/get_j_tags (decombine.py:820-866) and SeqIO.parse (:683-696)
 * produce for one chain.  Strings are NUL-terminated; regions may be any case
 * (the library upper-cases them like `.seq.upper()`, :695). */
typedef struct dcrx_tagset {
  uint32_t n_v;
  const char *const *v_tags;    /* v_seqs */
  const int32_t *v_jumps;       /* jump_to_end_v */
  const char *const *v_regions; /* v_regions */
  uint32_t n_j;
  const char *const *j_tags;    /* j_seqs */
  const int32_t *j_jumps;       /* jump_to_start_j */
  const char *const *j_regions; /* j_regions */
  int32_t v_half_split;         /* decombine.py:657-661 */
  int32_t j_half_split;
} dcrx_tagset_t;

typedef struct dcrx_tables dcrx_tables_t;

typedef struct dcrx_tables_info {
  uint32_t n_v, n_j;
  uint32_t n_states;        /* states of the merged V/J/half-tag automaton */
  uint32_t dfa_bytes;       /* bytes of the LDS-resident transition table */
  uint32_t n_keywords[6];   /* distinct keywords: V, J, V half1, V half2, J half1, J half2 */
  uint32_t max_tag_len;
  uint32_t tables_in_lds;   /* 1 when the transition table fits the LDS budget */
  uint32_t equal_len_per_automaton; /* 1 when every automaton's keywords share one length (acora tie order then irrelevant) */
  uint32_t pair_scan_bytes;  /* bytes of the two-bases-per-step table of the fast kernel; 0 = not built (> 4095 states,
                                or tags that overlap themselves at shifts 1..4) */
  uint32_t v2_tables;        /* 1 when the v2 kernels serve this tag set (every keyword class of one length, each
                                frame's automaton within 4095 states); else the three-launch form runs */
  uint32_t v2_states[2];     /* states of the forward- / reverse-frame automaton of the v2 scan */
  uint32_t v2_scan_bytes[2]; /* bytes of its 16-bit two-bases-per-step table (what the scan kernel keeps in LDS) */
  uint32_t max_read_len;     /* longest read a batch may hold (DCRX_E_UNSUPPORTED beyond) */
} dcrx_tables_info_t;

/* Compiles the six Aho-Corasick automata of decombine.py:722-746 into one merged
 * DFA plus the per-tag side tables.  Pure host work: needs no GPU.
 * DCRX_E_UNSUPPORTED when a tag is empty, longer than 32 nt, has a character
 * outside ACGT, a half split outside (0, len), a jump outside [-32768, 32767],
 * or the automaton needs more than 16383 states. */
int dcrx_tables_create(const dcrx_tagset_t *tagset, dcrx_tables_t **out);
void dcrx_tables_destroy(dcrx_tables_t *tables);
int dcrx_tables_info(const dcrx_tables_t *tables, dcrx_tables_info_t *info);

/* ---- per-read results: replaces dcr()'s return value (decombine.py:572-581) ---- */

/* 16 bytes per read.  When status == DCRX_S_OK:
 *   [v, j, vdel, jdel, frame_read[ins_start : ins_start+ins_len], v_start, j_end]
 * is exactly dcr()'s 7-list, with frame_read = revcomp(read) when frame == 0 and
 * read itself when frame == 1 (decombine.py:1015-1020).  Otherwise every field
 * but status/frame is 0 and status names the exit path (dcrx_codes.h). */
typedef struct dcrx_record {
  uint16_t v, j;
  uint16_t v_start, j_end;
  uint16_t ins_start, ins_len;
  uint8_t vdel, jdel;
  uint8_t status; /* enum dcrx_status */
  uint8_t frame;  /* 0 reverse, 1 forward */
} dcrx_record_t;

/* inputargs keys read on the path: orientation (:999-1010), allowNs (:554),
 * lenthreshold (:557) */
typedef struct dcrx_cfg {
  int32_t orientation; /* enum dcrx_orientation */
  int32_t allow_ns;
  int32_t lenthreshold;
  uint32_t flags;      /* DCRX_F_* */
} dcrx_cfg_t;

#define DCRX_F_NONE 0u
/* Every other bit of `flags` is a test or profiling switch of the library's own build (declared in the private header
 * decombinator_amd/csrc/dcrx_debug_flags.h, used by this repository's tests and tools).  The switches that leave the
 * records unchanged (A/B launch shapes) are honoured; those that make a kernel stop half-way (records are then NOT
 * results) are refused with DCRX_E_INVALID unless the environment holds DCRX_DEBUG_FLAGS=1.  A caller passes 0. */

/* A batch of reads, 2-bit packed: base i of read r is bits [2(i%4), 2(i%4)+1] of
 * byte packed[r*stride + i/4]; A=0 C=1 G=2 T=3.  Bytes of the FASTQ sequence that
 * are not one of "ACGT" (N, IUPAC codes, lower case) are packed as 0 and listed
 * as exceptions sorted by (read, pos); the device treats them exactly as the
 * reference treats the original byte.  stride is a multiple of
 * 8 with 4*stride >= the longest read and stride <= 16384: reads of up to 65 535 nt — the 16-bit
 * lengths, exception positions and record offsets of this ABI (DCRX_E_UNSUPPORTED beyond;
 * dcrx_tables_info.max_read_len; the reference itself has no limit, decombine.py:228-265).  By stride:
 * <= 40 (150 nt, two reads per lane in registers), <= 80 (320 nt) and <= 128 (511 nt, one read per lane)
 * run on the v2 kernels' register shapes (where those do not apply — dcrx_tables_info.v2_tables == 0 —
 * batches with stride > 80 take a kernel that walks the packed words in memory); a batch with a larger
 * stride takes the long form, one read per lane from memory, far slower per read: a caller puts its
 * reads of 512 nt and more into batches of their own (decombinator_amd/decombine.py does). */
typedef struct dcrx_batch {
  uint64_t n_reads;         /* < 2^32 per call */
  const uint8_t *packed;
  uint32_t stride;
  uint32_t read_len;        /* length of every read when lens == NULL */
  const uint16_t *lens;     /* optional per-read lengths */
  uint64_t n_exc;
  const uint32_t *exc_read; /* read index, ascending */
  const uint16_t *exc_pos;  /* position in the read as stored (FASTQ frame), ascending within a read */
  const uint8_t *exc_chr;   /* the original byte; never one of "ACGT" */
} dcrx_batch_t;

/* ---- host-side packing (the reads come from readfq, decombine.py:228-265) ---- */

/* Packs n_reads ASCII sequences (concatenated in `ascii`, read r at
 * [offsets[r], offsets[r+1])) into `packed` (n_reads*stride bytes) and `lens`.
 * Exceptions go to exc_* (capacity exc_cap).  Returns the number of exceptions
 * found (which may exceed exc_cap: call again with larger buffers), or a
 * negative dcrx_error. */
int64_t dcrx_pack_reads(const char *ascii, const uint64_t *offsets, uint64_t n_reads,
                        uint32_t stride, uint8_t *packed, uint16_t *lens,
                        uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr,
                        uint64_t exc_cap);

/* Same, for reads that are not contiguous: read r is ascii[start[r] .. start[r]+len[r]).
 * This is the form the batch reader below hands out (and the R1 mode's vdj = seq[bclength:],
 * decombine.py:980). */
int64_t dcrx_pack_reads_span(const char *ascii, const uint64_t *start, const uint32_t *len,
                             uint64_t n_reads, uint32_t stride, uint8_t *packed, uint16_t *lens,
                             uint32_t *exc_read, uint16_t *exc_pos, uint8_t *exc_chr,
                             uint64_t exc_cap);

/* Inverse of dcrx_pack_reads: writes lens[r] (or read_len) ASCII bytes of read r
 * to ascii + offsets[r], exception bytes restored. */
int dcrx_unpack_reads(const dcrx_batch_t *host_batch, const uint64_t *offsets, char *ascii);

/* ---- FASTQ / FASTA batch reader (host only) ----
 * Replaces the generator readfq (decombine.py:228-265) over the reference's opener
 * (opener_check, :118-123; text mode = universal newlines), record for record: header up to
 * the first space, multi-line sequences and qualities, FASTA records (no quality), a
 * truncated last record, and the l[:-1] quirk of an unterminated last line.  A batch is a
 * set of offsets into one text buffer owned by the reader, valid until the next call on the
 * same reader. */
typedef struct dcrx_fastq dcrx_fastq_t;

#define DCRX_FASTQ_NO_QUAL 0xFFFFFFFFu /* qual_len of a record the reference yields with qual None */

typedef struct {
  uint64_t n_records;
  const char *text;
  uint64_t text_bytes;
  const uint64_t *name_off; const uint32_t *name_len;
  const uint64_t *seq_off;  const uint32_t *seq_len;
  const uint64_t *qual_off; const uint32_t *qual_len;
} dcrx_fastq_batch_t;

/* gzipped != 0: the file must be gzip (gzip.open); 0: read as it is (open). */
int dcrx_fastq_open(const char *path, int gzipped, dcrx_fastq_t **out);
/* One rank's part of a sharded stage (no counterpart in the single-process reference; its order contract is the read loop's,
 * decombine.py:951-1050): the bytes [begin, end) of a plain four-line FASTQ file, `begin` a record's first byte — the reader
 * touches no other byte of the file, and fails (DCRX_E_INVALID) on anything but plain four-line records. */
int dcrx_fastq_open_range(const char *path, uint64_t begin, uint64_t end, dcrx_fastq_t **out);
/* Newlines among the bytes [begin, end) of a file; nth >= 1: *nth_off = the offset just behind the nth of them (UINT64_MAX when
 * there are fewer; with n_lines == NULL the scan stops there); *has_cr: a carriage return occurs; *file_size.  With it the
 * ranks agree on record boundaries (record k of a four-line file starts at line 4 k) while each reads only its own byte range. */
int dcrx_fastq_lines(const char *path, uint64_t begin, uint64_t end, uint64_t nth, uint64_t *n_lines, uint64_t *nth_off, int *has_cr,
                     uint64_t *file_size);
void dcrx_fastq_close(dcrx_fastq_t *reader);
/* Up to max_records further records; n_records == 0 means the file is exhausted. */
int dcrx_fastq_next(dcrx_fastq_t *reader, uint64_t max_records, dcrx_fastq_batch_t *out);

/* How many of the n spans hold `byte` within their first `prefix` bytes: the reference's
 * `"N" in bc` tally over bc = seq[:bclength] (decombine.py:985-989). */
uint64_t dcrx_count_prefix_byte(const char *text, const uint64_t *start, const uint32_t *len,
                                uint64_t n, uint32_t prefix, int byte);

/* ---- bulk `.n12` row assembly (host only) ----
 * Replaces the row building of the read loop (decombine.py:1012-1039) for a whole batch:
 * for every record with status DCRX_S_OK, in read order, one line
 *   v j vdel jdel insert id inter-tag-seq inter-tag-qual barcode barcode-qual [v_tail]
 * with the string `field_sep` (", " gives the `.n12` text itself, io.py:507-509) between fields
 * and '\n' after the row.  vdj / qual / id / bc / bcq / tail
 * give read r's strings as spans (tail may be NULL: no sampling_analysis).  The reverse frame
 * is revcomp(vdj) and qual[::-1] (:1015-1017); slices clamp like Python's.
 * Returns the number of bytes the rows take (computed without touching the text); they are
 * written only when out != NULL and that fits out_cap (call with out = NULL to size the buffer).  *n_rows = rows.  DCRX_E_UNSUPPORTED when a field
 * itself contains field_sep (or '\n' cannot occur: lines are split there). */
typedef struct {
  const char *text;
  const uint64_t *start;
  const uint32_t *len;
} dcrx_spans_t;

int64_t dcrx_assemble_rows(const dcrx_record_t *records, uint64_t n_reads, const dcrx_spans_t *vdj,
                           const dcrx_spans_t *qual, const dcrx_spans_t *id, const dcrx_spans_t *bc,
                           const dcrx_spans_t *bcq, const dcrx_spans_t *tail, const char *field_sep,
                           char *out, uint64_t out_cap, uint64_t *n_rows);

/* ---- the hot path: replaces the body of the read loop, decombine.py:998-1013 ---- */

/* Host buffers in, host buffers out (H2D copy, kernels, D2H copy, synchronous).
 * records: n_reads entries; counters: DCRX_N_COUNTERS uint64, OVERWRITTEN with
 * this batch's tallies (the caller adds them into its Counter).  The one-chain case of
 * dcrx_decombine_chains (the same chunk pipeline): the same bytes as dcrx_decombine_chains(&tables, 1, ...). */
int dcrx_decombine(dcrx_tables_t *tables, const dcrx_cfg_t *cfg, const dcrx_batch_t *host_batch,
                   dcrx_record_t *records, uint64_t *counters);

/* Several chains of one library (alpha + beta, gamma + delta) over ONE host batch: the host-buffer chunk pipeline with
 * one upload per chunk and n_chains resolutions of it (dcrx_decombine is its one-chain case).  Each chunk is copied in
 * once, into the staging of tables[0]; each chain's launches run on that handle's own stream, with its own workspace,
 * gated by an event on the copy in, and with several chains the same stream copies the chain's records and counters
 * out (one chain: the handle's copy-out stream) into records[c] (n_reads entries) and counters[c] (DCRX_N_COUNTERS
 * uint64, OVERWRITTEN).  An input staging set is refilled only once every chain's scan of it is over.
 * records[c] and counters[c] equal what dcrx_decombine(tables[c], ...) gives on the same batch, byte for byte.
 * Pinned caller buffers skip the staging copies as in dcrx_decombine; the tuple sink is off for the call on every
 * handle.  DCRX_E_INVALID for n_chains of 0 or above DCRX_MAX_CHAINS, a null pointer, or the same handle twice (the
 * chains would share one workspace).  Synchronous; on an error every stream has drained before this returns. */
#define DCRX_MAX_CHAINS 4
int dcrx_decombine_chains(dcrx_tables_t *const *tables, uint32_t n_chains, const dcrx_cfg_t *cfg,
                          const dcrx_batch_t *host_batch, dcrx_record_t *const *records, uint64_t *const *counters);

/* Device buffers in, device buffers out, asynchronous on `hip_stream`
 * (a hipStream_t, NULL = default stream).  Every pointer inside `device_batch`,
 * d_records and d_counters (DCRX_N_COUNTERS uint64, overwritten) are device
 * memory.  No allocation and no synchronisation happens inside once the tables
 * have been used on this device with a batch at least this large
 * (dcrx_reserve_device does that up front) — with ONE exception, and only where the caller has asked for it
 * (dcrx_set_tune_wait, below): the fourth call of a size class of 2^25 reads and more may then wait for the third
 * call's finishing launch, once per class.  Without that call nothing in here ever waits for the device, so the
 * stream may be captured or run arbitrarily far ahead of the host.
 * Calls on one handle are ordered on one stream (the workspace hangs off the handle); batches that should overlap —
 * a batch's finishing launch beside the next batch's scan, or the two chains of a two-chain library — take one handle
 * and one stream each ("Ownership, errors, threading"); dcrx_decombine_chains does that for host
 * buffers, uploading the batch once for all chains. */
int dcrx_decombine_device(dcrx_tables_t *tables, const dcrx_cfg_t *cfg,
                          const dcrx_batch_t *device_batch, dcrx_record_t *d_records,
                          uint64_t *d_counters, void *hip_stream);

/* ---- the DCR count of the barcode-free stage (decombine -nbc --count-dcrs): replaces the
 * reference's `Counter` over dcr() results that its non-barcode branch never filled
 * (decombine.py:1041-1060) ---- */

/* Opaque table of distinct DCRs, resident on the device it is first used on, growing across calls.  A DCR is
 * (v, j, vdel, jdel, insert) of a record with status DCRX_S_OK; insert is the frame read's bytes
 * [ins_start, ins_start + ins_len) exactly as the `.n12` row's fifth field holds them (exception bytes included,
 * complemented as revcomp() does in the reverse frame).  Each entry keeps the key, a 64-bit count and the smallest
 * read ordinal that carried the key.  Two DCRs are merged only when their full keys compare equal.  Like a tables
 * handle it is not thread-safe, and the steps that feed one table run on ONE stream.  Reset empties it and keeps its
 * device memory. */
typedef struct dcrx_counts dcrx_counts_t;
int dcrx_counts_create(dcrx_counts_t **out);
void dcrx_counts_destroy(dcrx_counts_t *counts);
int dcrx_counts_reset(dcrx_counts_t *counts);
/* Keeps only the low `bits` bits (0 .. 63; 63 by default) of every key's hash, on an empty table (after create or reset).
 * The results do not change: with few bits, distinct DCRs share hashes and every merge goes through the full-key
 * comparisons (the same hash inside a batch, a published slot of that hash in the table).  For tests; slower. */
int dcrx_counts_set_hash_bits(dcrx_counts_t *counts, uint32_t bits);

/* The count step (the primitive): adds the DCR of every OK record of d_records (device_batch->n_reads entries, device
 * memory) into `counts`, asynchronously on `hip_stream`.  device_batch is the batch those records came from (packed
 * reads, lengths, exceptions: device memory), as dcrx_decombine_device read it.  Read r's ordinal is
 * first_index + r, or first_index + d_index[r] when d_index (device, n_reads uint32) is given — for a batch that the
 * caller has split (reads over 511 nt in calls of their own).  The step aggregates a batch before it touches the
 * table: each distinct DCR of the batch costs one update of the table.  It allocates (and then synchronises the stream)
 * only when the table, the arena of inserts or its work space must grow. */
int dcrx_count_device(dcrx_counts_t *counts, const dcrx_record_t *d_records, const dcrx_batch_t *device_batch,
                      uint64_t first_index, const uint32_t *d_index, void *hip_stream);

/* dcrx_decombine with the count step on each chunk, on the same stream as the chunk's kernels: the records stay on the
 * device, only the counters (DCRX_N_COUNTERS uint64, OVERWRITTEN) come back.  Ordinals as in dcrx_count_device, with
 * `index` a host array of n_reads entries (or NULL).  Synchronous.  The one-chain case of dcrx_decombine_chains_count:
 * the same bytes as dcrx_decombine_chains_count(&tables, 1, ...). */
int dcrx_decombine_count(dcrx_tables_t *tables, const dcrx_cfg_t *cfg, const dcrx_batch_t *host_batch,
                         dcrx_counts_t *counts, uint64_t first_index, const uint32_t *index, uint64_t *counters);

/* dcrx_decombine_chains with the count step of chain c into counts[c] on that chain's stream, behind its kernels.  The
 * count step reads the packed chunk, so it is among the launches an input set waits for before it is refilled.
 * counts[c] and counters[c] equal what dcrx_decombine_count(tables[c], ..., counts[c], ...) gives on the same batch.
 * DCRX_E_INVALID for the same counts handle twice.  Synchronous. */
int dcrx_decombine_chains_count(dcrx_tables_t *const *tables, uint32_t n_chains, const dcrx_cfg_t *cfg,
                                const dcrx_batch_t *host_batch, dcrx_counts_t *const *counts, uint64_t first_index,
                                const uint32_t *index, uint64_t *const *counters);

/* The distinct DCRs of `counts` in collections.Counter.most_common() order over the reads in ordinal order: count
 * descending, ties by the smaller first ordinal.  Entry k: v[k], j[k], vdel[k], jdel[k], count[k], first[k] (its first
 * ordinal), and its insert ins_text[ins_off[k] .. ins_off[k + 1]) (ins_off: n + 1 entries, no terminator).  Returns n,
 * the number of distinct DCRs, and sets *text_bytes; writes the arrays only when cap >= n and text_cap >= *text_bytes
 * (call with cap = 0 to size them: that call only counts, it neither compacts nor sorts).  Synchronises the device. */
int64_t dcrx_counts_read(dcrx_counts_t *counts, uint16_t *v, uint16_t *j, uint8_t *vdel, uint8_t *jdel, uint64_t *count,
                         uint64_t *first, uint64_t *ins_off, char *ins_text, uint64_t cap, uint64_t text_cap,
                         uint64_t *text_bytes);

/* The `.nbc` text of n counted DCRs (what dcrx_counts_read gives): one line per DCR, "v j vdel jdel insert count" with
 * field_sep between the fields and '\n' after the line.  Returns the bytes the text takes; writes it only when out != NULL
 * and it fits out_cap.  A buffer of n * (DCRX_COUNTS_LINE_BOUND + 5 * strlen(field_sep)) + ins_off[n] - ins_off[0] bytes
 * always fits, and is written in one pass.  Host only. */
#define DCRX_COUNTS_LINE_BOUND 54   /* digits of v, j (5 each), vdel, jdel (3 each), count (20), and the newline */
int64_t dcrx_format_counts(uint64_t n, const uint16_t *v, const uint16_t *j, const uint8_t *vdel, const uint8_t *jdel,
                           const uint64_t *count, const uint64_t *ins_off, const char *ins_text, const char *field_sep,
                           char *out, uint64_t out_cap);

/* ---- the error merge of the barcode-free count (decombine -nbc --count-dcrs --merge-errors): low-count DCRs one or
 * two substitutions away from an abundant one are folded into it.  The reference has no counterpart (its -nbc loop
 * never runs, decombine.py:950, :1041-1060): the contract below is this library's own ---- */

#define DCRX_MERGE_ANCHOR 32         /* germline bases kept on either side of the junction */
#define DCRX_MERGE_MAX_JUNCTION 128  /* longest junction compared (256 bits at 2 bits a base) */

/* Input: n counted DCRs as dcrx_counts_read gives them (entry k has rank k: count descending, ties by first ordinal), the
 * chain's tables, a distance D (1 or 2) and a ratio R (>= 1).
 *   junction(e) = Vr[len(Vr) - aV : len(Vr) - vdel] + insert + Jr[jdel : aJ], with Vr / Jr the upper-cased regions of the
 *     entry's genes, aV = min(DCRX_MERGE_ANCHOR, len(Vr)), aJ likewise: the slice of the sequence translate rebuilds
 *     (V[:-vdel] + insert + J[jdel:]) between two anchors that depend on (v, j) only, so that a substitution the
 *     deletion walk turned into a larger vdel / jdel and a longer insert is still ONE mismatch between equal lengths.
 *   e is in reach when vdel <= aV, jdel <= aJ, the insert and both windows hold only ACGT (upper case) and the junction
 *     has at most DCRX_MERGE_MAX_JUNCTION bases.  An entry out of reach is never a child and never a parent.
 *   p is an eligible parent of c when both are in reach, v, j and the junction's length are equal,
 *     hamming(junction_c, junction_p) <= D, rank_p < rank_c and count_c <= count_p / R (integer division; the counts
 *     are the input's).  parent(c) is the eligible parent of the smallest rank, if any; root(c) follows the parent links to
 *     their end (so a child of a child joins the grandparent's tree although the two may be 2 D apart).
 * Output: one entry per root with its own key, the sum of its tree's counts and the smallest first ordinal of its tree,
 * ordered by count descending, then first ordinal, then rank.  A function of the input table alone. */
typedef struct dcrx_merge_stats {
  uint64_t entries_in;     /* n */
  uint64_t roots_out;      /* entries of the output */
  uint64_t out_of_reach;   /* entries the step left as they came */
  uint64_t merged;         /* entries that have a parent */
  uint64_t reads_moved;    /* sum of the merged entries' counts */
  uint64_t longest_chain;  /* most parent links between an entry and its root */
} dcrx_merge_stats_t;

/* Bytes of device work space dcrx_merge_parents_device needs for n entries. */
uint64_t dcrx_merge_work_bytes(uint64_t n);

/* The primitive: parent(c) of every entry, asynchronously on `hip_stream`, all arrays in device memory.  d_ins_off: n + 1
 * offsets into d_ins_text (text_bytes bytes; an entry whose insert would leave them counts as out of reach, as one whose
 * v or j the tables do not have).  d_parent[k] (n uint32) receives parent(k)'s rank, or k itself where there is none;
 * d_reach[k] (n bytes, may be NULL) 1 when entry k is in reach.  d_work: dcrx_merge_work_bytes(n) bytes, 256-byte
 * aligned, free for other use once the stream has passed the call.  The germline windows come from `tables` (uploaded on
 * the handle's first merge on a device: that call synchronises).  n < 2^31.  Encodes every junction (one lane per entry),
 * sorts the entries by (v, j, length) — stable, so a bucket stays in rank order — and searches each child's parent among
 * the head of its bucket: the entries that satisfy the ratio are a prefix of the bucket, staged in LDS tile by tile. */
int dcrx_merge_parents_device(dcrx_tables_t *tables, uint64_t n, const uint16_t *d_v, const uint16_t *d_j,
                              const uint8_t *d_vdel, const uint8_t *d_jdel, const uint64_t *d_count,
                              const uint64_t *d_ins_off, const char *d_ins_text, uint64_t text_bytes, uint32_t distance,
                              uint64_t ratio, uint32_t *d_parent, uint8_t *d_reach, void *d_work, uint64_t work_bytes,
                              void *hip_stream);

/* The whole step on host arrays, synchronous on the current device: uploads the table, runs the primitive, follows the
 * parent links to the roots (pointer jumping), adds each tree's counts and first ordinals onto its root (integer
 * atomics) and orders the roots.  root_of_out[k] (n): the rank of entry k's root (k itself for a root).  The output's
 * entry m (m < the return value) is input entry order_out[m] with count count_out[m] and first ordinal first_out[m]
 * (three arrays of n entries).  stats_out may be NULL.  Returns the number of roots, or a negative dcrx_error:
 * DCRX_E_INVALID for a v or j the tables do not have, offsets that go backwards, a distance outside 1 .. 2 or a ratio
 * of 0; DCRX_E_UNSUPPORTED for 2^31 entries or more; DCRX_E_HIP when the device cannot hold the table. */
int64_t dcrx_merge_dcrs(dcrx_tables_t *tables, uint64_t n, const uint16_t *v, const uint16_t *j, const uint8_t *vdel,
                        const uint8_t *jdel, const uint64_t *count, const uint64_t *first, const uint64_t *ins_off,
                        const char *ins_text, uint32_t distance, uint64_t ratio, uint32_t *root_of_out,
                        uint32_t *order_out, uint64_t *count_out, uint64_t *first_out, dcrx_merge_stats_t *stats_out);

/* The table of the roots out of the input table and what dcrx_merge_dcrs returned: output entry k (k < m) gets the key of
 * input entry order[k] — v, j, vdel, jdel and the insert's bytes, out_ins_off[0] = 0 .. out_ins_off[m] — in one pass.
 * out_ins_text holds at least the inserts' bytes of the whole input table.  Returns the bytes written to out_ins_text.
 * Host only. */
int64_t dcrx_merge_gather(uint64_t n, uint64_t m, const uint32_t *order, const uint16_t *v, const uint16_t *j,
                          const uint8_t *vdel, const uint8_t *jdel, const uint64_t *ins_off, const char *ins_text,
                          uint16_t *out_v, uint16_t *out_j, uint8_t *out_vdel, uint8_t *out_jdel, uint64_t *out_ins_off,
                          char *out_ins_text);

/* Profiling aid: the following dcrx_decombine_device calls on `tables` record
 * start_event right before and stop_event right after the dominant kernel (the scan),
 * on the stream that kernel is launched on (hipEvent_t handles, e.g. from
 * dcrx_event_create).  NULL, NULL switches it off. */
int dcrx_set_timing_events(dcrx_tables_t *tables, void *start_event, void *stop_event);

/* The same around EVERY launch of a dcrx_decombine_device call (prologue, scan, finishing kernels):
 * the time the whole hot path takes on the device for one batch. */
int dcrx_set_step_events(dcrx_tables_t *tables, void *start_event, void *stop_event);

/* Uploads the tables to the current device and sizes the per-launch workspace
 * for batches of up to max_reads reads.  Footprint (device memory, owned by the
 * handle until dcrx_tables_destroy): the entry lists between the kernels of a
 * call, ~109 bytes per read at stride <= 40 where the scan kernel takes the tail itself (pair tables of up to 64 KB:
 * 1.09 GB for 10 M reads of 150 nt, 10.9 GB for 100 M) and ~163 where the tail is a role of the finishing launch (the tail
 * list is allocated by the first call that needs it), ~310 bytes per read at stride <= 80 (none beyond stride 128: the
 * long form keeps no lists), plus max_reads / 8
 * bytes of exception bitmap, 8 bytes per read of hand-over queues and a few MB
 * of tables.  A later, larger batch grows it (synchronising the device). */
int dcrx_reserve_device(dcrx_tables_t *tables, uint64_t max_reads);

/* Compacts the status==OK records of a batch (the DCR tuples that are gathered
 * across GPUs): d_hits gets the records in input order, d_hit_index their read
 * indices (first_index + position), d_n_hits (one uint64) the count. */
int dcrx_compact_hits_device(const dcrx_record_t *d_records, uint64_t n_reads, uint64_t first_index,
                             dcrx_record_t *d_hits, uint64_t *d_hit_index, uint64_t *d_n_hits,
                             void *hip_stream);

/* Same compaction with the read indices as a bitmap instead of a list: bit (i & 63) of
 * d_ok_bitmap[i >> 6] is set when read i decombined ((n_reads + 63) / 64 words; the k-th record
 * of d_hits belongs to the k-th set bit).  A third fewer bytes to gather than 8-byte indices. */
int dcrx_compact_hits_bitmap_device(const dcrx_record_t *d_records, uint64_t n_reads,
                                    dcrx_record_t *d_hits, uint64_t *d_ok_bitmap, uint64_t *d_n_hits,
                                    void *hip_stream);

/* The same with each decombined record squeezed into 12 bytes (three little-endian uint32; offsets of nine bits: batches of
 * reads of up to 511 nt only):
 *   word 0: v (bits 0-11) | j (12-23) | vdel (24-31)
 *   word 1: v_start (0-8) | j_end (9-17) | ins_start (18-26)
 *   word 2: ins_len (0-8) | jdel (9-16) | frame (17)
 * status is DCRX_S_OK by construction.  Requires < 4096 V and J tags (any real tag set) and reads of up to 511 nt (positions
 * < 512).  d_tuples12: 12 bytes per record. */
int dcrx_compact_hits_packed_device(const dcrx_record_t *d_records, uint64_t n_reads, void *d_tuples12,
                                    uint64_t *d_ok_bitmap, uint64_t *d_n_hits, void *hip_stream);

/* The same in 8 bytes per decombined record (two little-endian uint32), what a sharded run gathers on rank 0:
 *   word 0: v (bits 0-10) | j (11-19) | vdel (20-27) | jdel low 4 bits (28-31)
 *   word 1: jdel high 4 bits (0-3) | v_start (4-12) | j_end (13-21) | ins_len (22-30) | frame (31)
 * ins_start is not sent: it is the base after the end of V (decombine.py:547, :577), v_start + jump_to_end_v[v] - vdel, which
 * the receiver has from the tag file.  Requires < 2048 V tags and < 512 J tags (any real tag set; dcrx_tables_info gives
 * the counts); positions are < 512 by the read-length limit. */
int dcrx_compact_hits_packed8_device(const dcrx_record_t *d_records, uint64_t n_reads, void *d_tuples8,
                                     uint64_t *d_ok_bitmap, uint64_t *d_n_hits, void *hip_stream);

/* The narrow tuple: what a sharded run gathers when the receiver holds the same tag tables.  Field widths come from the
 * tables (dcrx_tuple_layout), fields are packed least significant first:
 *   v | j | vdel | jdel | v_start | j_end | short_end | frame
 * w_v / w_j: bits of n_v - 1 / n_j - 1; w_vdel: bits of max(jump_to_end_v[k] - len(v_seqs[k])) and w_jdel: bits of
 * max(jump_to_start_j[k]) — a decombined read has passed the filter of decombine.py:560-564, so its deletions fit; w_pos
 * (v_start and j_end): bits of max_read_len.  Neither ins_start nor ins_len is sent:
 *   ins_start = v_start + jump_to_end_v[v] - vdel                       (the base after the end of V, :283-285, :547)
 *   ins_len   = j_end - L - jump_to_start_j[j] + jdel - ins_start       (start of J, :407-409, :447, :506-509, :806)
 * with L = len(j_seqs[j]), or 2 * j_half_split when short_end is set: the J half1 rescue sets j_seq_end to the half's
 * start + len(half1) + j_half_split (:450-454), which is not the tag's end when the split is not the tag's middle.
 * bits = the sum (+ 2); bytes = max(4, ceil(bits / 8)) <= 8.  Human beta, original tags, 150 nt: 39 bits, 5 bytes.
 * DCRX_E_UNSUPPORTED when bits > 64 (the caller gathers 12-byte tuples instead).
 * Contract: every read of a batch whose tuples are packed with a layout is at most 2^w_pos - 1 bases long (max_read_len
 * fits by construction).  dcrx_decombine_device refuses a batch that can break it while a tuple sink is set (DCRX_E_INVALID:
 * read_len, or 4 * stride for a batch with lens); dcrx_compact_hits_narrow_device sees records only and trusts its caller. */
typedef struct dcrx_tuple_layout {
  uint8_t w_v, w_j, w_vdel, w_jdel, w_pos;
  uint8_t bits, bytes, reserved;
  uint32_t max_read_len;
} dcrx_tuple_layout_t;
int dcrx_tuple_layout(const dcrx_tables_t *tables, uint32_t max_read_len, dcrx_tuple_layout_t *layout);

/* Bytes of the message of a batch over n_reads read slots with n_hits decombined ones (dcrx_compact_hits_narrow_device):
 *   [ (n_reads + 63) / 64 uint64: bit (i & 63) of word i >> 6 = read i decombined ]
 *   [ n_hits uint32: the tuples' low 32 bits, in read order ]
 *   [ n_hits x (bytes - 4) bytes: their high bytes, least significant first ]
 * The third part starts where the second ends: a sender ships the first dcrx_tuple_message_bytes(...) bytes. */
uint64_t dcrx_tuple_message_bytes(const dcrx_tuple_layout_t *layout, uint64_t n_reads, uint64_t n_hits);

/* Compacts the status==OK records of a batch into that message (d_message: room for n_hits == n_reads); d_n_hits (one
 * uint64) gets the count.  n_slots >= n_reads: the read slots the bitmap spans — a sharded run sizes every step's message
 * for its largest batch, a short last batch leaves the bits beyond its reads zero.  Needs the tables on the current
 * device (the J tags' lengths and jumps decide short_end). */
int dcrx_compact_hits_narrow_device(dcrx_tables_t *tables, const dcrx_tuple_layout_t *layout,
                                    const dcrx_record_t *d_records, uint64_t n_reads, uint64_t n_slots, void *d_message,
                                    uint64_t *d_n_hits, void *hip_stream);

/* The tuple sink of a handle: while one is set, every dcrx_decombine_device call on the handle ALSO leaves the batch's
 * message — exactly what dcrx_compact_hits_narrow_device would make of its records, n_slots >= the batch's reads — in
 * d_message and the count in d_n_hits, on the call's stream.  For the shipped kernels and tuples of up to 40 bits the
 * kernels that write the records leave the tuples behind as they go and one short launch behind them puts the message in
 * read order (no pass over the records: the gather of a sharded run costs the step ~2 %, not 12 %); any other launch
 * shape compacts the records behind the call.  The buffers may change from call to call (a sharded run alternates two
 * messages); layout == NULL turns the sink off.  The handle's workspace grows by ~32 bytes per read of its largest batch. */
int dcrx_set_tuple_sink(dcrx_tables_t *tables, const dcrx_tuple_layout_t *layout, void *d_message, uint64_t n_slots,
                        uint64_t *d_n_hits);

/* ---- the first consumer of the rows: the front half of `collapse` (host, threaded) -------------------------------
 * What read_in_data (src/decombinator/collapse.py:482-565) does to every `.n12` row before it starts grouping rows:
 * get_barcode_positions :367-479 (spacer searches :192-236), set_barcode :278-326, check_umi_quality :343-353 and the
 * inter-tag length filter :553-556, with the reference's counter keys.  `text`: rows as dcrx_assemble_rows writes them
 * (fields separated by cfg->field_sep, one row per line).  Per row a dcrx_collapse_row_t; counters are ADDED to
 * counters[DCRX_CF_N_COUNTERS].  All three spacer searches of the reference are decided here: the spacer verbatim, with up
 * to two substitutions ("{1s<=2}"), and the indel form ("{2i+2d+1s<=2}", :198-201: the spacer with one base inserted or one
 * deleted, the leftmost start first, the insertion where both hold).  DCRX_CF_DEFER (nothing counted) is left for rows
 * that are not ten fields of ASCII text: the caller's own error path.  rows == NULL: returns the number of rows.
 * row_offsets (optional, n + 1 entries): where each row starts in `text`.  Returns the number of rows or an error. */
enum dcrx_collapse_status { DCRX_CF_OK = 0, DCRX_CF_NO_BCLOCS = 1, DCRX_CF_LOW_QUALITY = 2, DCRX_CF_OVERLONG = 3, DCRX_CF_DEFER = 255 };
enum dcrx_collapse_counter {
  DCRX_CF_C_INPUT_DCRS = 0,        /* readdata_input_dcrs */
  DCRX_CF_C_FAIL_N = 1,            /* getbarcode_fail_N */
  DCRX_CF_C_FAIL_NOSPACER = 2,     /* getbarcode_fail_nospacerfound */
  DCRX_CF_C_FAIL_NOT2SPACERS = 3,  /* getbarcode_fail_not2spacersfound */
  DCRX_CF_C_FAIL_N1SHORT = 4,      /* getbarcode_fail_n1tooshort */
  DCRX_CF_C_FAIL_N1LONG = 5,       /* getbarcode_fail_n1toolong */
  DCRX_CF_C_FAIL_N2PASTEND = 6,    /* getbarcode_fail_n2pastend */
  DCRX_CF_C_PASS_EXACT = 7,        /* getbarcode_pass_exactmatch */
  DCRX_CF_C_PASS_REGEX = 8,        /* getbarcode_pass_regexmatch */
  DCRX_CF_C_PASS_FUZZY_RIGHTLEN = 9, /* getbarcode_pass_fuzzymatch_rightlen */
  DCRX_CF_C_PASS_FUZZY_SHORT = 10, /* getbarcode_pass_fuzzymatch_short */
  DCRX_CF_C_PASS_FUZZY_LONG = 11,  /* getbarcode_pass_fuzzymatch_long */
  DCRX_CF_C_PASS_OTHER = 12,       /* getbarcode_pass_other */
  DCRX_CF_C_FAIL_NO_BCLOCS = 13,   /* readdata_fail_no_bclocs */
  DCRX_CF_C_SHORT_BARCODE = 14,    /* readdata_short_barcode */
  DCRX_CF_C_LONG_BARCODE = 15,     /* readdata_long_barcode */
  DCRX_CF_C_FAIL_LOW_QUALITY = 16, /* readdata_fail_low_barcode_quality */
  DCRX_CF_C_FAIL_OVERLONG = 17,    /* readdata_fail_overlong_intertag_seq */
  DCRX_CF_C_SUCCESS = 18,          /* readdata_success */
  DCRX_CF_N_COUNTERS = 19
};
typedef struct dcrx_collapse_cfg {
  int32_t oligo;            /* 0 m13, 1 i8, 2 i8_single, 3 nebio, 4 takara (collapse.py:174-189) */
  int32_t allow_ns;         /* inputargs["allowNs"] (:390) */
  int32_t lenthreshold;     /* inputargs["lenthreshold"] (:553) */
  double min_bc_q, bc_q_below_min, avg_q_threshold; /* barcode_quality_parameters (:343-353) */
  char field_sep[8];        /* NUL-terminated; ", " for `.n12` text */
} dcrx_collapse_cfg_t;
typedef struct dcrx_collapse_row {
  int16_t b1start, b1end, b2start, b2end; /* bc_locs (b2start = b2end = -1 for nebio / takara), -1 when none */
  uint8_t status;                          /* enum dcrx_collapse_status */
  uint8_t barcode_len, barcode_qual_len;
  uint8_t pad;
  char barcode[24], barcode_qual[24];      /* set_barcode's two strings */
} dcrx_collapse_row_t;
/* spacerSearch (collapse.py:204-212) on its own: every non-overlapping match of `spacer` in seq[0, n), left to right, found by
 * the first of the three searches that finds any — regex.findall(spacer, seq), "(spacer){1s<=2}", "(spacer){2i+2d+1s<=2}".
 * starts[k] / lens[k] (up to `cap` of them) receive the matches; *kind: 0 verbatim, 1 substitutions, 2 indel.  Returns the
 * number of matches (it may exceed cap) or an error. */
int32_t dcrx_spacer_search(const char *seq, int32_t n, const char *spacer, int32_t m, int32_t *starts, int32_t *lens, int32_t cap,
                           int32_t *kind);
int64_t dcrx_collapse_front(const char *text, uint64_t n_bytes, const dcrx_collapse_cfg_t *cfg, dcrx_collapse_row_t *rows,
                            uint64_t rows_cap, uint64_t *row_offsets, uint64_t *counters, int n_threads);

/* ---- the intermediate files' gzip step (reference io.py:497-506: the text re-read and written through gzip.open) ----
 * A multi-member gzip file whose pieces (4 MB of text each) are deflated by n_threads threads (0: the host's); any gzip
 * reader sees one stream with exactly the bytes written.  level 1..9 (the reference's gzip.open uses 9).
 * Errors (a path that cannot be opened, a short write) are DCRX_E_INVALID with the text in dcrx_last_error(). */
int dcrx_gzip_open(const char *path, int level, int n_threads, void **writer);
int dcrx_gzip_write(void *writer, const void *data, uint64_t n_bytes);
int dcrx_gzip_close(void *writer);

/* ---- stage 2 of `collapse`: UMI neighbour search (GPU), grouping and counting (host) -------------------------------
 * The reference's make_merge_groups (src/decombinator/collapse.py:723-751) asks pyrepseq.nn.symdel for every pair of
 * distinct UMIs within Levenshtein distance `bcthreshold`, then keeps the upper triangle in ascending (i, j) order.  Here:
 *
 *   dcrx_umi_encode            host: UMIs (ASCII + offsets) -> records sorted by (length, composition), one per UMI, and a
 *                              summary per tile of DCRX_UMI_TILE records (the device search's input)
 *   dcrx_umi_neighbours_device device buffers in, asynchronous on `hip_stream`: every pair within distance k as a 64-bit
 *                              key (i << 32 | j, i < j, original indices), in no particular order; up to pair_cap of them
 *                              are written and *d_total receives the number found (zeroed by the call itself)
 *   dcrx_umi_neighbours        host convenience: encode, search on the current device, sort.  Returns the number of pairs;
 *                              when it exceeds pair_cap nothing is written to `pairs` and the caller calls again with room
 *                              for that many (as dcrx_pack_reads)
 *
 * Limits: a UMI is at most DCRX_UMI_MAX_LEN bytes (what dcrx_collapse_row_t.barcode holds) and one call sees at most
 * DCRX_UMI_MAX_SYMBOLS distinct byte values (A, C, G, T, N, and the S / L of set_barcode fit); beyond either the call
 * returns DCRX_E_UNSUPPORTED.  Any k >= 0: a k above DCRX_UMI_MAX_LEN is taken as DCRX_UMI_MAX_LEN on entry (no two UMIs
 * are farther apart, so the pairs are the same), which keeps the search's int32 arithmetic in k in range. */
#define DCRX_UMI_MAX_LEN 24
#define DCRX_UMI_MAX_SYMBOLS 8
#define DCRX_UMI_TILE 256
#define DCRX_UMI_REC_WORDS 16   /* per record: Peq[8], packed codes[3], length, composition[2], original index, pad */
#define DCRX_UMI_TILE_WORDS 8   /* per tile: min length, max length, composition minima[2], maxima[2], record count, pad */
/* The records (n_tiles * DCRX_UMI_TILE of them, the tail padded) and tiles of n UMIs; returns n_tiles, or an error.
 * recs == NULL: only checks the limits and returns n_tiles. */
int64_t dcrx_umi_encode(const char *ascii, const uint64_t *offsets, uint64_t n, uint32_t *recs, uint32_t *tiles);
int dcrx_umi_neighbours_device(const uint32_t *d_recs, const uint32_t *d_tiles, uint64_t n_tiles, int32_t k,
                               uint64_t *d_pairs, uint64_t pair_cap, uint64_t *d_total, void *hip_stream);
int64_t dcrx_umi_neighbours(const char *ascii, const uint64_t *offsets, uint64_t n, int32_t k, uint64_t *pairs,
                            uint64_t pair_cap);

/* Grouping (read_in_data, collapse.py:585-683), over the rows dcrx_collapse_front left (status DCRX_CF_OK join groups;
 * DCRX_CF_OVERLONG rows count towards the input DCRs only, :555-563), in input order: a barcode has at most one group
 * (index 0); a read joins it when are_seqs_equivalent(protoseq, seq, lev_fraction) (:349-354), else the barcode turns
 * multi-TCR for good; the protoseq is the group's most common seq (ties: the first seen); a changed protoseq re-keys the
 * group, which moves it to the end of the reference's dict.  `text` and the row offsets must outlive the handle.
 * counters[DCRX_GRP_N_COUNTERS] receive the reference's keys below. */
enum dcrx_group_counter {
  DCRX_GRP_C_KEYS = 0,            /* readdata_barcode_dcretc_keys */
  DCRX_GRP_C_INPUT_UNIQUE = 1,    /* number_input_unique_dcrs */
  DCRX_GRP_C_INPUT_TOTAL = 2,     /* number_input_total_dcrs */
  DCRX_GRP_C_MULTI_BARCODES = 3,  /* multi_tcr_barcodes */
  DCRX_GRP_C_MULTI_READS = 4,     /* multi_tcr_barcode_reads */
  DCRX_GRP_N_COUNTERS = 5
};
typedef struct dcrx_groups dcrx_groups_t;
int dcrx_collapse_group(const char *text, uint64_t n_bytes, const uint64_t *row_offsets, const dcrx_collapse_row_t *rows,
                        uint64_t n_rows, const char *field_sep, double lev_fraction, int sampling_analysis,
                        dcrx_groups_t **groups, uint64_t *counters);
void dcrx_groups_destroy(dcrx_groups_t *groups);
/* Sizes: groups, member rows, bytes of all UMIs, bytes of all protoseqs. */
int dcrx_groups_info(const dcrx_groups_t *groups, uint64_t *n_groups, uint64_t *n_members, uint64_t *umi_bytes,
                     uint64_t *proto_bytes);
/* In group order: the UMIs and protoseqs (text + n_groups + 1 offsets each; any may be NULL) and each group's member rows
 * (member_off: n_groups + 1 entries; member_rows: input row indices in join order). */
int dcrx_groups_export(const dcrx_groups_t *groups, char *umi_text, uint64_t *umi_off, char *proto_text, uint64_t *proto_off,
                       uint64_t *member_off, uint64_t *member_rows);
/* keep[e] = are_seqs_equivalent(protoseq of group a, of group b, lev_fraction) for the pairs (a, b) = (pairs[e] >> 32,
 * pairs[e] & 0xffffffff) — make_clusters' edge test (collapse.py:771-779). */
int dcrx_groups_equivalent(const dcrx_groups_t *groups, const uint64_t *pairs, uint64_t n_pairs, double lev_fraction,
                           uint8_t *keep, int n_threads);
/* collapsinate (collapse.py:897-977) over clusters given as group lists in concatenation order
 * (cluster c = cluster_groups[cluster_off[c] .. cluster_off[c + 1])): each cluster votes for its most common DCR (ties: the
 * first seen), DCRs in order of their first cluster.  Per DCR: votes[d], size_sum[d] (reads of its clusters); freq_text
 * receives the `.freq` lines "v, j, vdel, jdel, insert, count, round(mean cluster size)" (round half to even).
 * Pass freq_text == NULL to learn *n_dcrs and *freq_bytes first.  With extra != 0 also *wc_bytes / wc_text (the
 * write_clusters lines, :813-843, without the header) and *bd_bytes / bd_text (the -bd lines, :959-967). */
int dcrx_collapse_count(const dcrx_groups_t *groups, const uint32_t *cluster_groups, const uint64_t *cluster_off,
                        uint64_t n_clusters, uint64_t *n_dcrs, uint64_t *votes, uint64_t *size_sum, uint64_t *freq_bytes,
                        char *freq_text, int extra, uint64_t *wc_bytes, char *wc_text, uint64_t *bd_bytes, char *bd_text);
/* are_seqs_equivalent on its own (tests): 1 when levenshtein(a, b) <= len(shorter) * lev_fraction. */
int dcrx_seqs_equivalent(const char *a, uint32_t na, const char *b, uint32_t nb, double lev_fraction);

/* ---- translate.get_cdr3 for a batch of DCRs (host only) ----
 * Replaces the per-row body of the reference's CDR3 step (src/decombinator/translate.py:257-357, called per unique DCR from
 * cdr3translator :388-533): from the gene tables of import_gene_information (:163-254) and the five fields of each DCR,
 *   sequence = V region without its last vdel bases + insert + J region from base jdel on (:296-305), its translation
 *   (standard table; codons with IUPAC ambiguity codes as Bio.Seq.translate resolves them), the in-frame, stop-codon,
 *   conserved-C and conserved-F calls (:312-347) and, for productive rows, where junction_aa / junction lie (:350-355).
 * Every index and slice behaves as Python's.  Strings travel as one text and offsets: gene k's region is
 * v_regions[v_region_off[k] .. v_region_off[k + 1]) (upper case, as the reference stores them), likewise the V genes'
 * conserved residues (v_translate_residue: compared as a whole string with ONE residue of the translation, :327) and the J
 * genes' motifs (j_translate_residue: searched with re.findall in four residues, :341-343 — literal characters, '.',
 * character classes and escaped literals are served here; a motif with any other regular-expression syntax is parsed only when a
 * row uses its gene, as the reference compiles only the motif it searches with, and such a row comes back DCRX_CDR3_MOTIF_LEFT:
 * text, in_frame, stop, conserved_c, start_cdr3 are set, productive holds the calls so far, junction_aa_off / junction_aa_len
 * say which residues of sequence_aa the search looks at, and the caller finishes the row with its own engine — conserved_f,
 * end_cdr3 = len(sequence_aa[start_cdr3:]) + j_pos + start_cdr3 + 1 on a match, the junctions; decombinator_amd/translate.py does).
 * The DCRs: v / j / vdel / jdel as integers (int(dcr[k]), :283-286), the insert of row r = ins[ins_off[r] .. ins_off[r + 1])
 * (the caller has stripped the blank the `translate` command's rows carry, :287-290).
 * Returns the bytes the rows' text takes — per row its sequence, then its sequence_aa — written into `text` when that fits
 * text_cap (call with text = NULL to size the buffer); rows[r] says where they lie.  A row the reference would raise on keeps
 * status != 0 and nothing else: DCRX_CDR3_INDEX_ERROR (a gene index outside its table, or a translation shorter than the V
 * gene's residue position: IndexError), DCRX_CDR3_BAD_CODON (a letter that is no nucleotide code: Biopython's "Codon '...'
 * is invalid", bad_codon_at = the codon's first base; a codon of three gaps '---' is the gap '-', as Seq.translate has it). */
enum dcrx_cdr3_status { DCRX_CDR3_OK = 0, DCRX_CDR3_INDEX_ERROR = 1, DCRX_CDR3_BAD_CODON = 2, DCRX_CDR3_MOTIF_LEFT = 3 };
typedef struct dcrx_cdr3_genes {
  uint32_t n_v, n_j;
  const char *v_regions; const uint64_t *v_region_off;      /* n_v + 1 offsets */
  const char *j_regions; const uint64_t *j_region_off;      /* n_j + 1 */
  const int32_t *v_pos; const char *v_res; const uint32_t *v_res_off;        /* v_translate_position, v_translate_residue */
  const int32_t *j_pos; const char *j_motif; const uint32_t *j_motif_off;    /* j_translate_position, j_translate_residue */
} dcrx_cdr3_genes_t;
typedef struct dcrx_cdr3_row {
  uint64_t seq_off, aa_off;              /* into the text: sequence, sequence_aa */
  uint32_t seq_len, aa_len;
  uint32_t junction_off, junction_len;          /* inside the row's sequence (productive rows; else 0, 0) */
  uint32_t junction_aa_off, junction_aa_len;    /* inside the row's sequence_aa */
  int32_t start_cdr3, end_cdr3;          /* as the reference computes them (residues) */
  uint32_t bad_codon_at;
  uint8_t status;                        /* enum dcrx_cdr3_status */
  uint8_t productive, in_frame, stop, conserved_c, conserved_f;      /* 1 = "T" */
  uint8_t pad[2];
  uint32_t reserved;                     /* (64 bytes) */
} dcrx_cdr3_row_t;
int64_t dcrx_cdr3_batch(const dcrx_cdr3_genes_t *genes, uint64_t n, const int32_t *v, const int32_t *j, const int32_t *vdel,
                        const int32_t *jdel, const char *ins, const uint64_t *ins_off, dcrx_cdr3_row_t *rows, char *text, uint64_t text_cap);

/* ---- clonotypes (`translate --clonotypes`, `pipeline --clonotypes`): the counted DCRs translated and grouped by
 * (V call, J call, CDR3 amino acids) on the GPU.  The reference stops at one AIRR row per DCR and has no counterpart: the
 * contract below is this library's own.  The entries only ADD to ABI 5 (nothing that existed changes) ----
 *
 * Input: a counted table of n entries (v, j, vdel, jdel, insert, count) — entry k has rank k — and a gene set: the tables of
 * dcrx_cdr3_genes_t with one call group per gene (genes whose names up to the '*' are equal share a group; the caller
 * numbers the groups).
 * Per entry: the calls of dcrx_cdr3_batch, exactly — status, in_frame, stop, conserved_c, conserved_f, productive,
 *   start_cdr3, end_cdr3, seq_len, aa_len, bad_codon_at, junction_aa_off / _len, junction_off / _len — and for a productive
 *   entry the bytes of junction_aa and junction.  Python's index and slice rules, Biopython's rules for ambiguity codes and
 *   gaps, lower case and IUPAC bytes of an insert as dcrx_cdr3_batch documents them.  dcrx_cdr3_batch itself is untouched
 *   and shares no code with these entries: it is what they are tested against.
 * Member: an entry with status OK that is productive.  Non-productive entries and entries with status INDEX_ERROR or
 *   BAD_CODON are left out and counted in the statistics.  An entry with status MOTIF_LEFT (its J gene's motif needs a
 *   regular-expression engine) makes dcrx_clonotypes return DCRX_E_UNSUPPORTED: there is no CPU fallback.
 * Clonotype: the members whose keys (V call group, J call group, junction_aa bytes) compare equal in full, whatever the
 *   junction's length.  A 64-bit hash of the key only sorts candidates next to each other: a hash match alone never merges.
 * Output, one row per clonotype: duplicate_count = the sum of its members' counts (64 bits), n_dcrs = the number of members,
 *   the representative = the member with the largest count (ties: the smallest rank) and that count.  Rows are ordered by
 *   duplicate_count descending, then the representative's rank ascending.  clonotype_of[k] = the row of entry k, UINT32_MAX
 *   for a non-member.  The result is a function of the input table and the gene set alone: no launch shape, tile size or
 *   hash width enters it (integer adds, max and min only), and the duplicate_counts add up to the members' counts. */
typedef struct dcrx_clono_genes dcrx_clono_genes_t;

/* The gene set: the tables are copied, compiled (per V gene its frame-0 translation with its first stop and first invalid
 * codon, per J gene and phase the translation and "next stop / invalid codon at or after codon k", the motifs as byte
 * classes) and uploaded once, on the handle's first use on a device; the handle then belongs to that device (DCRX_E_INVALID on
 * another: create a handle per device).  Not thread-safe.  v_group / j_group: n_v / n_j call
 * groups.  DCRX_E_UNSUPPORTED when the tables pass 2^31 bytes. */
int dcrx_clono_genes_create(const dcrx_cdr3_genes_t *genes, const uint32_t *v_group, const uint32_t *j_group,
                            dcrx_clono_genes_t **out);
void dcrx_clono_genes_destroy(dcrx_clono_genes_t *genes);
/* Keeps only the low `bits` bits (0 .. 64; 64 by default) of every key's hash in dcrx_clonotypes.  The results do not
 * change: with few bits distinct keys share hashes and the full comparisons decide every merge.  For tests; slower. */
int dcrx_clono_set_hash_bits(dcrx_clono_genes_t *genes, uint32_t bits);

/* One entry as the device leaves it (32 bytes).  flags: bit 0 productive, 1 in_frame, 2 stop, 3 conserved_c, 4 conserved_f.
 * The other fields of dcrx_cdr3_row_t follow from these, with s[a:b] Python's slice of a string of that length:
 *   aa_len = seq_len / 3; status BAD_CODON: bad_codon_at = (uint32_t)start_cdr3 (nothing else is set, as in dcrx_cdr3_batch);
 *   productive and status OK: junction_aa = sequence_aa[start_cdr3 : end_cdr3], junction = sequence[3 start_cdr3 : 3 end_cdr3];
 *   hash = the clonotype key's hash, arena_off = where junction_aa, then junction, lie in the arena (else both 0);
 *   status MOTIF_LEFT: the motif window is sequence_aa[start_cdr3:][j_pos : j_pos + 4]. */
typedef struct dcrx_clono_row {
  uint64_t hash, arena_off;
  int32_t start_cdr3, end_cdr3;
  uint32_t seq_len;
  uint8_t status, flags;
  uint16_t pad;
} dcrx_clono_row_t;

/* Bytes of device work space dcrx_cdr3_device needs for n entries whose inserts take text_bytes bytes. */
uint64_t dcrx_clono_work_bytes(uint64_t n, uint64_t text_bytes);

/* The primitive: the calls of every entry, asynchronously on `hip_stream`, all arrays in device memory.  d_v, d_j, d_vdel,
 * d_jdel: n int32 each, as dcrx_cdr3_batch takes them; d_ins_off: n + 1 offsets into d_ins_text (text_bytes bytes; an entry
 * whose insert would leave them gets status INDEX_ERROR).  d_rows: n rows.  The junction bytes of the productive entries go
 * into d_arena at exact offsets, back to back in rank order, nothing truncated: a lengths pass, an exclusive scan, then a
 * write pass (the write pass re-reads an entry through the gene tables, which costs a few look-ups per residue; a fixed slot
 * per entry would pay for the longest junction n times).  *d_arena_need (device, uint64) receives the bytes the arena takes;
 * an entry whose bytes would pass arena_cap is not written, so a caller that finds *d_arena_need > arena_cap calls again
 * with a larger arena (d_arena may be NULL with arena_cap 0 to size it).  d_work: dcrx_clono_work_bytes(n, text_bytes)
 * bytes, 256-byte aligned; a smaller one is DCRX_E_INVALID, not a launch.  n < 2^30. */
int dcrx_cdr3_device(dcrx_clono_genes_t *genes, uint64_t n, const int32_t *d_v, const int32_t *d_j, const int32_t *d_vdel,
                     const int32_t *d_jdel, const uint64_t *d_ins_off, const char *d_ins_text, uint64_t text_bytes,
                     dcrx_clono_row_t *d_rows, char *d_arena, uint64_t arena_cap, uint64_t *d_arena_need, void *d_work,
                     uint64_t work_bytes, void *hip_stream);

typedef struct dcrx_clonotype_stats {
  uint64_t entries_in, reads_in;
  uint64_t productive, productive_reads;            /* the members */
  uint64_t nonproductive, nonproductive_reads;      /* status OK, not productive */
  uint64_t untranslatable, untranslatable_reads;    /* status INDEX_ERROR or BAD_CODON */
  uint64_t clonotypes_out;
  uint64_t convergent;                              /* clonotypes with n_dcrs > 1 */
  uint64_t largest_n_dcrs;
} dcrx_clonotype_stats_t;

/* The whole step on host arrays, synchronous on the current device: uploads the table, runs the primitive with an arena of
 * the exact size, sorts the members by (hash, rank) — a stable radix sort —, compares every member's key in full with the
 * head of its run (members that differ are resolved exactly, in rounds among themselves), adds the totals onto the heads
 * (integer atomics whose results are not read) and orders the rows with two stable radix sorts.  Row r (r < the return
 * value): rep_out[r] = the representative's rank, dup_out[r], ndcrs_out[r], top_out[r] = the representative's count; its
 * junction_aa is text[junc_off_out[2 r] .. junc_off_out[2 r + 1]) and its junction text[junc_off_out[2 r + 1] ..
 * junc_off_out[2 r + 2]) of the text dcrx_clonotypes_text gives.  The five arrays hold n entries (junc_off_out 2 n + 1),
 * clonotype_of_out n; stats_out may be NULL.  Returns the number of clonotypes or a negative dcrx_error: DCRX_E_UNSUPPORTED
 * for a MOTIF_LEFT entry (the message names the J gene and its motif) and for 2^30 entries or more, DCRX_E_INVALID for
 * offsets that go backwards. */
int64_t dcrx_clonotypes(dcrx_clono_genes_t *genes, uint64_t n, const int32_t *v, const int32_t *j, const int32_t *vdel,
                        const int32_t *jdel, const uint64_t *count, const uint64_t *ins_off, const char *ins_text,
                        uint32_t *rep_out, uint64_t *dup_out, uint32_t *ndcrs_out, uint64_t *top_out, uint64_t *junc_off_out,
                        uint32_t *clonotype_of_out, dcrx_clonotype_stats_t *stats_out);
/* The junction text of the handle's last dcrx_clonotypes: returns its bytes, copied to `out` when they fit `cap`. */
int64_t dcrx_clonotypes_text(dcrx_clono_genes_t *genes, char *out, uint64_t cap);

/* The `.clonotypes.tsv` text of m rows in one pass: a header line, then per row
 * "v_call j_call junction_aa duplicate_count n_dcrs junction decombinator_id top_dcr_count", tab separated; v_call / j_call
 * are the representative's gene's call (calls: one text, n_genes + 1 offsets), decombinator_id its "v, j, vdel, jdel, insert".
 * Returns the bytes the text takes; writes it when out != NULL and it fits out_cap.  Host only. */
int64_t dcrx_format_clonotypes(uint64_t m, const uint32_t *rep, const uint64_t *dup, const uint32_t *ndcrs, const uint64_t *top,
                               const uint64_t *junc_off, const char *junc_text, uint64_t n, const int32_t *v, const int32_t *j,
                               const int32_t *vdel, const int32_t *jdel, const uint64_t *ins_off, const char *ins_text,
                               uint32_t n_v, const char *v_calls, const uint32_t *v_call_off, uint32_t n_j, const char *j_calls,
                               const uint32_t *j_call_off, char *out, uint64_t out_cap);

/* ---- the CDR3 network (`--clonotypes --cdr3-network`): which clonotypes lie one or two CDR3 residues apart, and the
 * clusters they form, on the GPU.  The reference has no counterpart: the contract below is this library's own.  The entries
 * only ADD to ABI 5 (nothing that existed changes) ----
 *
 * This layer knows nothing about genes: it works on NODES, which the caller makes out of a clonotype table.
 * Input: m nodes — node i has rank i — with, per node, a class c_i (uint32), a string s_i (bytes, given as m + 1 offsets
 *   into one text) and a weight w_i (uint64); and a distance D, 1 or 2.
 * In reach: 1 <= len(s_i) <= DCRX_CDR3NET_MAX_LEN (32).  A node out of reach (empty, or longer) has no neighbours: it is a
 *   cluster of its own, and it is counted.  The limit is a design choice: 32 bytes are eight dwords of registers per lane,
 *   as the error merge keeps its junction; real CDR3 junctions have 8 to 25 residues.
 * Edge: {i, j}, i != j, where both nodes are in reach, c_i == c_j, len(s_i) == len(s_j) and the Hamming distance of the
 *   bytes is <= D.  Bytes are compared as they are: upper case, lower case, 'X', '*' and bytes >= 0x80 are each equal to
 *   themselves alone.  Distance 0 is an edge (two clonotypes of one CDR3 that the classes do not separate).
 * Output: degree[i]; the adjacency in CSR form, adj_off[m + 1] (uint64) and adj[] with every node's neighbours' ranks
 *   ascending; cluster_of[i] = the row of i's connected component; per cluster row head = its smallest rank, n_nodes, and
 *   weight = the sum of its nodes' weights.  Cluster rows are ordered by head ascending (a clonotype table is ordered by
 *   abundance: clusters come in the order of their most abundant clonotype).
 * The result is a function of the input alone: no tile size, launch shape or order of arrival enters it (integer adds, min
 *   and max, and atomics whose results are not read). */
#define DCRX_CDR3NET_MAX_LEN 32

/* Bytes of device work space dcrx_cdr3_neighbours_device needs for m nodes whose strings take text_bytes bytes; 0 for
 * m >= 2^30. */
uint64_t dcrx_cdr3net_work_bytes(uint64_t m, uint64_t text_bytes);

/* The primitive: degree and adjacency of every node, asynchronously on `hip_stream`, all arrays in device memory.  d_class:
 * m classes; d_off: m + 1 offsets into d_text (text_bytes bytes; a node whose offsets go backwards or leave the text is out
 * of reach).  Writes d_degree (m) and d_adj_off (m + 1: the exclusive sum of the degrees in rank order).  *d_adj_need
 * (device, uint64) always receives the entries the adjacency takes (= d_adj_off[m], twice the number of edges); d_adj
 * (adj_cap entries) is written when the need fits adj_cap and is never written past otherwise (an entry beyond adj_cap is
 * dropped), so a caller that finds *d_adj_need > adj_cap calls again with a larger one (d_adj may be NULL with adj_cap 0 to
 * size it).  The steps: keys, a stable radix sort of (key, rank) — a bucket stays in rank order —, the packed strings
 * gathered in sorted order, a degree pass in which a block of 256 sorted nodes walks the entries of its buckets in LDS
 * tiles of 256 (every node counts its own neighbours over its whole bucket: no atomics, neighbours in ascending rank), the
 * exclusive sum, and a write pass that repeats the walk.  d_work: dcrx_cdr3net_work_bytes(m, text_bytes) bytes, 256-byte
 * aligned; a smaller one is DCRX_E_INVALID, not a launch.  distance other than 1 or 2: DCRX_E_INVALID.  m < 2^30
 * (DCRX_E_UNSUPPORTED beyond). */
int dcrx_cdr3_neighbours_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                                uint64_t text_bytes, uint32_t distance, uint32_t *d_degree, uint64_t *d_adj_off, uint32_t *d_adj,
                                uint64_t adj_cap, uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream);

/* Nothing that depends on the algorithm is in here (the number of component rounds is not). */
typedef struct dcrx_cdr3_network_stats {
  uint64_t nodes_in;
  uint64_t out_of_reach;
  uint64_t edges;                 /* unordered pairs */
  uint64_t clusters_out;
  uint64_t singletons;            /* clusters of one node */
  uint64_t largest_cluster;       /* the largest n_nodes */
  uint64_t largest_degree;
} dcrx_cdr3_network_stats_t;

/* The whole step on host arrays, synchronous on the current device: uploads the nodes, runs the primitive's two halves
 * (the degree pass sizes the adjacency, which is then allocated — DCRX_E_NOMEM when it cannot be — and filled), then the
 * connected components — label[i] = i, rounds of "the smallest label among my neighbours and me" followed by pointer
 * jumping until a round changes nothing (one 4-byte copy back per round): the label is then the component's smallest rank —
 * and the totals: integer adds of weights and node counts onto the heads, whose results are not read, the heads compacted in
 * rank order.  degree_out, cluster_of_out: m entries; head_out, n_nodes_out, weight_out: m entries, of which the return value
 * are rows.  The adjacency is copied back only where it is asked for: adj_off_out (m + 1) may be NULL, and adj_out
 * (adj_cap entries) is filled when adj_off_out is given and the need fits adj_cap; *adj_need_out (may be NULL) receives the
 * need either way, so a caller that wants the edges calls once to size them.  stats_out may be NULL.  Returns the number of
 * clusters or a negative dcrx_error: DCRX_E_UNSUPPORTED for m >= 2^30, DCRX_E_INVALID for a distance other than 1 or 2 and
 * for offsets that go backwards, DCRX_E_NOMEM (after the degree pass) for an adjacency that cannot be allocated. */
int64_t dcrx_cdr3_network(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                          uint32_t distance, uint32_t *degree_out, uint32_t *cluster_of_out, uint32_t *head_out,
                          uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out, uint32_t *adj_out, uint64_t adj_cap,
                          uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out);

/* The `.cdr3_clusters.tsv` text of m nodes in one pass: a header line, then per node, in rank order,
 * "clonotype v_call j_call junction_aa duplicate_count cluster cluster_size cluster_duplicate_count degree", tab separated:
 * clonotype = the rank, v_call / j_call = the calls of v_idx[i] / j_idx[i] (calls: one text, n + 1 offsets), junction_aa =
 * the node's string, duplicate_count = its weight, cluster = cluster_of[i], and that row's n_nodes and weight.  Returns the
 * bytes the text takes; writes it when out != NULL and it fits out_cap.  Host only. */
int64_t dcrx_format_cdr3_clusters(uint64_t m, const uint32_t *v_idx, const uint32_t *j_idx, uint32_t n_v, const char *v_calls,
                                  const uint32_t *v_call_off, uint32_t n_j, const char *j_calls, const uint32_t *j_call_off,
                                  const uint64_t *off, const char *text, const uint64_t *weight, const uint32_t *cluster_of,
                                  uint64_t n_clusters, const uint32_t *n_nodes, const uint64_t *cluster_weight,
                                  const uint32_t *degree, char *out, uint64_t out_cap);
/* The `.cdr3_edges.tsv` text of a CSR adjacency in one pass: the header "a b distance", then one line per edge with a < b,
 * ascending by (a, b); the distance is computed here from the two strings.  Same return rule.  Host only. */
int64_t dcrx_format_cdr3_edges(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off, const char *text,
                               char *out, uint64_t out_cap);

/* ---- the CDR3 network's metric (`--cdr3-metric`): the contract above with a METRIC beside the distance.  The entries only
 * ADD to ABI 5; the four entries above keep their signatures and behaviour ----
 *
 * DCRX_CDR3NET_HAMMING (0): the contract above, and the default.  Every *_metric entry below then gives bit for bit what
 *   its counterpart above gives.
 * DCRX_CDR3NET_LEVENSHTEIN (1): CDR3 junctions are made by deleting germline ends and inserting nucleotides, so two related
 *   clonotypes differ by a gained or lost residue as often as by a substituted one.  Under this metric:
 * In reach: unchanged, 1 <= len(s_i) <= DCRX_CDR3NET_MAX_LEN (32).  A node out of reach has no neighbours.
 * Edge: {i, j}, i != j, where both nodes are in reach, c_i == c_j, |len(s_i) - len(s_j)| <= D and the Levenshtein distance
 *   of the bytes is <= D (D = 1 or 2).  Substitution, insertion and deletion cost 1 each.  Bytes are compared as they are:
 *   a real 0x00 byte is a symbol like any other and never matches the padding behind a shorter string.  Distance 0 is an
 *   edge.
 * Output, statistics, limits and error codes: unchanged — degree, the CSR with every node's neighbours' ranks ascending,
 *   cluster_of, cluster rows by head ascending, dcrx_cdr3_network_stats_t.  The result is a function of the input alone.
 * Any other metric is DCRX_E_INVALID.
 * The steps under DCRX_CDR3NET_LEVENSHTEIN: the bucket is the class alone — the stable sort of (key, rank) runs over the
 *   key's class bits and its out-of-reach bit only, so a class stays in rank order and the sorted keys keep every node's
 *   length —, a 32-bit letter-presence mask (bit byte & 31) is gathered beside every packed string, and the walk's pair test
 *   is: equal class, lengths at most D apart, presence masks at most 2 D bits apart (a filter: one substitution moves two of
 *   those bits at most, one insertion or deletion one), then an exact register-only edit-distance test (furthest-reaching
 *   rows on the 2 D + 1 diagonals, csrc/dcrx_cdr3net_core.h), which a lane runs on the entry it has waiting once some lane
 *   of its wave meets its next one, so that many lanes run it together. */
#define DCRX_CDR3NET_HAMMING 0
#define DCRX_CDR3NET_LEVENSHTEIN 1

/* dcrx_cdr3net_work_bytes for a metric (the Levenshtein walk keeps a presence mask per node beside what the Hamming walk
 * keeps); 0 for m >= 2^30 and for a metric that does not exist. */
uint64_t dcrx_cdr3net_metric_work_bytes(uint64_t m, uint64_t text_bytes, uint32_t metric);

/* dcrx_cdr3_neighbours_device under `metric`: the same arguments, rules and errors; d_work takes
 * dcrx_cdr3net_metric_work_bytes(m, text_bytes, metric) bytes. */
int dcrx_cdr3_neighbours_metric_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                                       uint64_t text_bytes, uint32_t distance, uint32_t metric, uint32_t *d_degree,
                                       uint64_t *d_adj_off, uint32_t *d_adj, uint64_t adj_cap, uint64_t *d_adj_need, void *d_work,
                                       uint64_t work_bytes, void *hip_stream);

/* dcrx_cdr3_network under `metric`: the same arguments, rules and errors. */
int64_t dcrx_cdr3_network_metric(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                                 uint32_t distance, uint32_t metric, uint32_t *degree_out, uint32_t *cluster_of_out,
                                 uint32_t *head_out, uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out,
                                 uint32_t *adj_out, uint64_t adj_cap, uint64_t *adj_need_out, dcrx_cdr3_network_stats_t *stats_out);

/* dcrx_format_cdr3_edges under `metric`: with DCRX_CDR3NET_LEVENSHTEIN the distance column is the Levenshtein distance of the
 * two strings, computed here on the host (a plain two-row table), and an edge between strings of two lengths is not refused. */
int64_t dcrx_format_cdr3_edges_metric(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off,
                                      const char *text, uint32_t metric, char *out, uint64_t out_cap);

/* ---- overlap (`overlap`): which clonotypes several samples share, and how alike two repertoires are, on the GPU.  The
 * reference has no counterpart: the contract below is this library's own.  The entries only ADD to ABI 5 ----
 *
 * This layer knows nothing about genes or files: it works on ROWS, which the caller makes out of clonotype tables.
 * Input: S samples, 1 <= S <= DCRX_OVERLAP_MAX_SAMPLES (64: a design choice — a group's cells then take six key bits, a
 *   lane walks at most 63 later cells, and the pair kernel's per-block planes fit 64 KB of LDS); m rows, m < 2^30 — row i has
 *   rank i — with, per row, a sample (uint32 < S), a class (uint32), a string (bytes of any length, 0 included, given as
 *   m + 1 offsets into one text) and a weight (uint64).  A sample may have no row.
 * Key: (class, bytes), compared in full.  Bytes are compared as they are, and the length is part of the key ("CASS" is not
 *   "CASSL").  A 64-bit hash only puts candidates next to each other; dcrx_overlap_set_hash_bits is the test knob, and the
 *   result does not depend on it.
 * Group: the rows with one key.  Its head is its row of the smallest rank; groups are numbered by head ascending, and
 *   group_of[i] is row i's group.
 * Cell: (group, sample), with weight = the sum of that sample's rows in the group (several rows of one sample may share a
 *   key; they add).  Every row weight and every cell weight must be < 2^32 (DCRX_E_UNSUPPORTED otherwise; a cell sum that
 *   crosses the limit is found on the device by a flag that travels with the copy-back of the number of cells).  A group's
 *   n_samples is its number of cells.
 * Matrices: DCRX_OVERLAP_PLANES planes of S x S uint64, plane p's value at (a, b) at planes[(p * S + a) * S + b].  Every
 *   value is an exact integer and a function of the input alone.  For a != b the sums run over the groups that have a cell in
 *   both a (weight w_a) and b (weight w_b):
 *     DCRX_OVERLAP_SHARED         the number of such groups            (a, a): the sample's groups
 *     DCRX_OVERLAP_SHARED_WEIGHT  sum of w_a (not symmetric)           (a, a): the sample's reads X_a
 *     DCRX_OVERLAP_MIN_WEIGHT     sum of min(w_a, w_b)                 (a, a): X_a
 *     DCRX_OVERLAP_PROD_LO        sum of (w_a w_b mod 2^32)            (a, a): the same of w_a^2
 *     DCRX_OVERLAP_PROD_HI        sum of (w_a w_b >> 32)               (a, a): the same of w_a^2
 *   A product fits 64 bits because cells are < 2^32, and each half-sum stays < 2^62 because there are fewer than 2^30 groups:
 *   the caller composes prod_hi * 2^32 + prod_lo as a big integer (it may pass 2^64).
 * Public rows: the groups with n_samples >= min_samples (>= 1), ordered by three stable sorts from the least to the most
 *   significant key: head ascending, total weight descending, n_samples descending.  Each row carries head, n_samples,
 *   weight (the sum of its cells) and its cells as CSR: cell_off (rows + 1), cell_sample ascending, cell_weight.
 * Statistics: dcrx_overlap_stats_t and the rows per sample; nothing that depends on the algorithm is in there. */
#define DCRX_OVERLAP_MAX_SAMPLES 64
enum dcrx_overlap_plane {
  DCRX_OVERLAP_SHARED = 0,
  DCRX_OVERLAP_SHARED_WEIGHT = 1,
  DCRX_OVERLAP_MIN_WEIGHT = 2,
  DCRX_OVERLAP_PROD_LO = 3,
  DCRX_OVERLAP_PROD_HI = 4,
  DCRX_OVERLAP_PLANES = 5
};
typedef struct dcrx_overlap_stats {
  uint64_t rows_in;
  uint64_t groups;
  uint64_t private_groups;        /* groups of one sample */
  uint64_t shared_groups;         /* groups of two samples or more */
  uint64_t in_all_samples;        /* groups with a cell in every one of the S samples */
  uint64_t largest_n_samples;
  uint64_t public_rows;
  uint64_t public_cells;
} dcrx_overlap_stats_t;
typedef struct dcrx_overlap dcrx_overlap_t;

/* How many bits of the 64-bit key hash the grouping sorts by, 0 .. 64 (default 64; process wide, for tests: with 0 bits
 * every row is a candidate of every other and there are as many rounds of full compares as distinct keys).  DCRX_E_INVALID
 * above 64. */
int dcrx_overlap_set_hash_bits(uint32_t bits);

/* The whole step on host arrays, synchronous on the current device, run ONCE whatever is exported afterwards: the rows are
 * uploaded; overlap_keys_kernel hashes (class, bytes); a stable radix sort of (hash, rank), run heads, and rounds of full-key
 * compares against the first active row of every run (one round in practice) give the groups; a stable sort of
 * (group, sample) over at most 36 bits, run heads and integer atomics whose results are not read give the cells, compacted in
 * order; dcrx_overlap_pairs_device gives the planes; flag, compaction, the stable sorts and a gather give the public rows.
 * Returns the result, to be released with dcrx_overlap_destroy, or NULL with the dcrx_error in *error_out (may be NULL) and
 * its text in dcrx_last_error(): DCRX_E_INVALID for S of 0 or above DCRX_OVERLAP_MAX_SAMPLES, a sample id >= S, offsets that
 * go backwards, min_samples of 0 or a null argument; DCRX_E_UNSUPPORTED for m >= 2^30 and for a row or cell weight >= 2^32;
 * DCRX_E_NOMEM as elsewhere.  m == 0 is a result without groups (and touches no device). */
dcrx_overlap_t *dcrx_overlap_run(uint32_t n_samples, uint64_t m, const uint32_t *sample, const uint32_t *cls,
                                 const uint64_t *off, const char *text, const uint64_t *weight, uint32_t min_samples,
                                 int *error_out);
void dcrx_overlap_destroy(dcrx_overlap_t *overlap);
/* Sizes (samples, rows, public rows, public cells) and statistics; any pointer may be NULL. */
int dcrx_overlap_info(const dcrx_overlap_t *overlap, uint32_t *n_samples, uint64_t *n_rows, uint64_t *n_public,
                      uint64_t *n_public_cells, dcrx_overlap_stats_t *stats);
/* Into the caller's arrays, any of which may be NULL: planes (DCRX_OVERLAP_PLANES x S x S), group_of (rows),
 * rows_per_sample (S), the public rows' head, n_samples and weight (public rows each), cell_off (public rows + 1),
 * cell_sample and cell_weight (public cells each). */
int dcrx_overlap_export(const dcrx_overlap_t *overlap, uint64_t *planes, uint32_t *group_of, uint64_t *rows_per_sample,
                        uint32_t *head, uint32_t *n_samples, uint64_t *weight, uint64_t *cell_off, uint32_t *cell_sample,
                        uint64_t *cell_weight);

/* The primitive — the pair accumulation alone —, asynchronous on `hip_stream`, all arrays in device memory: cells in group
 * order (group g's are d_cell_off[g] .. d_cell_off[g + 1]; n_groups + 1 offsets, fewer than 2^30 cells), samples ascending
 * inside a group and < n_samples, weights < 2^32.  ADDS onto d_planes (DCRX_OVERLAP_PLANES x S x S uint64), which the caller
 * has zeroed (or not: what is there stays under the sums).  One lane per cell adds its diagonal terms and walks the later
 * cells of its own group (adjacent, at most 63; a group may straddle a block boundary: the walk reads global memory), adding
 * the five terms of each pair to the block's planes in LDS; one flush per block follows, by global 64-bit atomic adds whose
 * results are not read.  The planes are taken in two launches (shared + shared_weight + min_weight, then the two product
 * planes), the symmetric ones kept as triangles, so that a block's LDS stays under 64 KB at 64 samples; a group of one cell
 * costs its diagonal update and no walk.  DCRX_E_INVALID for n_samples of 0 or above DCRX_OVERLAP_MAX_SAMPLES or a null
 * argument, DCRX_E_UNSUPPORTED for 2^30 groups or more. */
int dcrx_overlap_pairs_device(uint64_t n_groups, const uint32_t *d_cell_off, const uint32_t *d_cell_sample,
                              const uint32_t *d_cell_weight, uint32_t n_samples, uint64_t *d_planes, void *hip_stream);

/* The `overlap_public.tsv` text of n_public rows in one pass: the header "v_call j_call junction_aa n_samples
 * duplicate_count" followed by one column per sample (its name), then per row the calls of its head row (v_idx / j_idx of
 * the m input rows into calls tables: one text, n + 1 offsets), the head row's string, n_samples, weight and per sample the
 * cell's weight or 0, tab separated.  Returns the bytes the text takes; writes it when out != NULL and it fits out_cap.
 * Host only. */
int64_t dcrx_format_overlap_public(uint64_t n_public, const uint32_t *head, const uint32_t *n_samples, const uint64_t *weight,
                                   const uint64_t *cell_off, const uint32_t *cell_sample, const uint64_t *cell_weight,
                                   uint32_t n_sample_names, const char *sample_names, const uint32_t *sample_name_off,
                                   uint64_t m, const uint32_t *v_idx, const uint32_t *j_idx, uint32_t n_v, const char *v_calls,
                                   const uint32_t *v_call_off, uint32_t n_j, const char *j_calls, const uint32_t *j_call_off,
                                   const uint64_t *off, const char *text, char *out, uint64_t out_cap);

/* ---- downsample (`overlap --downsample`, `overlap --diversity`): a subsample of every sample's reads without replacement,
 * to one depth, and the abundance classes a diversity table is computed from, on the GPU.  The reference has no counterpart:
 * the contract below is this library's own.  The entries only ADD to ABI 5 ----
 *
 * Input: S samples, 1 <= S <= DCRX_DOWNSAMPLE_MAX_SAMPLES (4096: a design choice — a sample keeps a histogram of 32 KB and as
 *   many bytes of candidate keys in the work space); m rows, m < 2^30, each a (sample uint32 < S, weight uint64) pair, the
 *   sample ids non-decreasing (DCRX_E_INVALID otherwise); a depth per sample (uint64); one 64-bit seed.
 * Reads: X_s is the sum of sample s's weights; the sum of X_s over all samples is below 2^40 (DCRX_E_UNSUPPORTED otherwise).
 *   The reads of sample s are numbered r = 0 .. X_s - 1 in row order: row i owns [P_i, P_i + w_i), P the exclusive sum of the
 *   weights inside the sample.
 * Key of a read, all arithmetic mod 2^64:
 *     fin(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     key(s, r) = fin( fin(seed + (s + 1) * 0xD1B54A32D192ED03) + (r + 1) * 0x9E3779B97F4A7C15 )
 *   fin is a bijection (xor-shifts and odd multipliers are), and the multiplier of r + 1 is odd, so the keys of one sample are
 *   pairwise distinct: there are no ties and no tie rule.  A counter-based hash and not a cryptographic generator is a design
 *   choice: every read's key is computed where it is needed, in any order, by any number of lanes; nobody is to be kept from
 *   predicting a subsample.
 * Kept: n_s = min(depth_s, X_s).  If n_s = X_s every read of the sample is kept and threshold[s] = 2^64 - 1.  Otherwise T_s is
 *   the (n_s + 1)-th smallest key of the sample and the kept reads are those with key < T_s: exactly n_s of them.
 * Output, each a function of the input alone (integer arithmetic only; no tile size, launch shape or order of arrival enters
 *   it): kept[i] = the kept reads of row i; reads[s] = X_s; depth_used[s] = n_s; threshold[s] = T_s.
 * A sample without rows, a row of weight 0 and a depth of 0 are valid. */
#define DCRX_DOWNSAMPLE_MAX_SAMPLES 4096

/* Bytes of device work space dcrx_downsample_device needs for m rows of n_samples samples; 0 for m >= 2^30 and for a number of
 * samples outside 1 .. DCRX_DOWNSAMPLE_MAX_SAMPLES. */
uint64_t dcrx_downsample_work_bytes(uint64_t m, uint32_t n_samples);

/* The primitive, asynchronous on `hip_stream`, all arrays in device memory: d_sample and d_weight m entries, d_depth,
 * d_reads, d_depth_used and d_threshold n_samples entries, d_kept m entries.  Nothing is copied back and nothing waits.
 * The steps: an exclusive sum of the weights gives the offsets of one index space over the reads of all samples; the space is
 * cut into tiles of 2048 consecutive reads, a block takes a run of tiles, finds a tile's first row by a search over the
 * offsets and stages the 512 offsets behind it in LDS (the work is split by reads, never by rows: a row of any weight costs
 * what its reads cost).  Selection: a histogram pass over the keys' top 12 bits (LDS histograms, flushed by integer atomics
 * whose results are not read) finds the bin of every sample's threshold; while a bin holds more than 4096 keys a further pass
 * on the next 12 bits follows for the samples concerned (none for samples below 16 million reads or so; the launches of a
 * level nobody needs return at once); the keys of the bin are written out, and the threshold is the one with the wanted
 * number of smaller keys.  A count pass evaluates the keys once more and adds, per run of a wave's lanes that fall in one
 * row, one number onto kept[row].  Keys are never stored for all reads.
 * d_work: dcrx_downsample_work_bytes(m, n_samples) bytes, 256-byte aligned; a smaller one is DCRX_E_INVALID, not a launch.
 * DCRX_E_INVALID for a number of samples outside 1 .. DCRX_DOWNSAMPLE_MAX_SAMPLES or a null argument, DCRX_E_UNSUPPORTED
 * for m >= 2^30.  What only the device can see: sample ids that are not non-decreasing below n_samples are outside the
 * contract (nothing is read or written outside the arrays); a sum of the weights of 2^40 or more leaves reads[] as summed and
 * kept, depth_used and threshold 0. */
int dcrx_downsample_device(uint32_t n_samples, uint64_t m, const uint32_t *d_sample, const uint64_t *d_weight,
                           const uint64_t *d_depth, uint64_t seed, uint64_t *d_kept, uint64_t *d_reads, uint64_t *d_depth_used,
                           uint64_t *d_threshold, void *d_work, uint64_t work_bytes, void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays of the same shapes: checks the arguments (all of the
 * contract's refusals, before any device call), uploads, runs the primitive on the null stream, copies back.  m == 0 is
 * answered on the host (every sample: 0 reads, depth_used 0, threshold 2^64 - 1) and touches no device. */
int dcrx_downsample(uint32_t n_samples, uint64_t m, const uint32_t *sample, const uint64_t *weight, const uint64_t *depth,
                    uint64_t seed, uint64_t *kept_out, uint64_t *reads_out, uint64_t *depth_used_out, uint64_t *threshold_out);

/* The abundance classes of samples (count of counts): n items, n < 2^30, each (sample < n_samples, group uint32, weight
 * uint64), 1 <= n_samples <= DCRX_OVERLAP_MAX_SAMPLES.  The items of one (sample, group) add into a cell; a cell sum of 2^32
 * or more is DCRX_E_UNSUPPORTED; a cell of weight 0 is dropped.  Per sample the distinct cell weights ascending, each with the
 * number of cells that have it, as CSR: sample s's classes are class_off_out[s] .. class_off_out[s + 1] (n_samples + 1
 * entries) of class_count_out (the weight) and class_mult_out (the cells), which hold n entries each.  Returns the number
 * of classes or a negative dcrx_error.  Synchronous on the current device, host arrays: a stable radix sort by
 * (sample, group), run heads and integer adds onto the heads whose results are not read give the cells; a sort by (sample,
 * weight), run heads and an ordered compaction give the classes.  n == 0 touches no device. */
int64_t dcrx_abundance_classes(uint32_t n_samples, uint64_t n, const uint32_t *sample, const uint32_t *group,
                               const uint64_t *weight, uint64_t *class_off_out, uint32_t *class_count_out,
                               uint64_t *class_mult_out);

/* ---- match (`match`): which nodes of one table (the QUERIES: a sample's clonotypes) are the same as, or one or two residues
 * from, a node of a second table (the TARGETS: a database of CDR3s of known specificity, or another sample), on the GPU.  The
 * reference has no counterpart: the contract below is this library's own.  The entries only ADD to ABI 5 ----
 *
 * This layer knows nothing about genes or files, as the CDR3 network's.
 * Input: m_t targets — target j has rank j — with, per target, a class c_j (uint32) and a string s_j (bytes, given as
 *   m_t + 1 offsets into one text); m_q queries — query i has rank i — with a class, a string and a weight w_i (uint64);
 *   a distance D, 0, 1 or 2; a metric, DCRX_CDR3NET_HAMMING or DCRX_CDR3NET_LEVENSHTEIN.  m_q, m_t < 2^30
 *   (DCRX_E_UNSUPPORTED beyond).  The sum of the query weights is below 2^64 (DCRX_E_UNSUPPORTED otherwise, decided on the
 *   host before any device call: no t_weight can wrap).
 * In reach: the network's rule, 1 <= len <= DCRX_CDR3NET_MAX_LEN (32), on either side.  A node out of reach takes part in
 *   no hit, and is counted.
 * Hit: (i, j) where query i and target j are both in reach, c_i == c_j, and the network's edge rule holds between the two
 *   strings: under DCRX_CDR3NET_HAMMING equal lengths and at most D differing bytes; under DCRX_CDR3NET_LEVENSHTEIN lengths
 *   at most D apart and a Levenshtein distance (substitution, insertion, deletion cost 1 each) of at most D.  Bytes are
 *   compared as they are; a real 0x00 byte is a symbol like any other and never matches the padding behind a shorter
 *   string.  D = 0 is byte equality under either metric.  A query and a target of the same bytes are a hit: the two sides
 *   are different sets, there is no "i != j".
 * Output: degree[i] = the hits of query i; the hits in CSR form, hit_off[m_q + 1] (uint64) and hit[] with every query's
 *   targets' ranks ascending; per target t_queries[j] = the queries that hit it (uint32) and t_weight[j] = the sum of their
 *   weights (uint64).  Statistics: dcrx_cdr3_match_stats_t, which holds nothing of the algorithm.
 * Everything is a function of the input alone (integer adds, and atomics whose results are not read).
 * D above 2, a metric that does not exist and offsets that go backwards are DCRX_E_INVALID. */
typedef struct dcrx_cdr3_index dcrx_cdr3_index_t;
typedef struct dcrx_cdr3_match dcrx_cdr3_match_t;
typedef struct dcrx_cdr3_match_stats {
  uint64_t queries;
  uint64_t targets;
  uint64_t queries_out_of_reach;
  uint64_t targets_out_of_reach;
  uint64_t hits;                  /* (query, target) pairs */
  uint64_t queries_hit;           /* queries with a hit ... */
  uint64_t queries_hit_weight;    /* ... and the sum of their weights */
  uint64_t targets_hit;           /* targets with a hit */
  uint64_t largest_degree;
} dcrx_cdr3_match_stats_t;

/* The targets, built on the current device ONCE and kept there for any number of dcrx_cdr3_match_run / _device calls (host
 * arrays; synchronous).  The index holds the targets in both bucket orders — by (class, length) for the Hamming walk and by
 * class alone for the Levenshtein walk, each a stable radix sort of (key, rank), so a bucket stays in rank order —: per
 * order the sorted keys, the ranks and the packed strings (32 bytes each), and for the class order the letter-presence
 * masks, which are always built: one index serves both metrics and every D, at 92 bytes per target.  m_t == 0 is a valid
 * index (and touches no device).  DCRX_E_UNSUPPORTED for m_t >= 2^30, DCRX_E_INVALID for offsets that go backwards or a
 * null argument, DCRX_E_NOMEM as elsewhere. */
int dcrx_cdr3_index_create(uint64_t m_t, const uint32_t *cls, const uint64_t *off, const char *text,
                           dcrx_cdr3_index_t **index_out);
void dcrx_cdr3_index_destroy(dcrx_cdr3_index_t *index);
/* The targets, how many of them are out of reach, and the index's bytes of device memory; any pointer may be NULL. */
int dcrx_cdr3_index_info(const dcrx_cdr3_index_t *index, uint64_t *targets, uint64_t *out_of_reach, uint64_t *device_bytes);

/* Bytes of device work space dcrx_cdr3_match_device needs for m_q queries whose strings take text_bytes bytes under `metric`
 * (it does not depend on the index); 0 for m_q >= 2^30 and for a metric that does not exist. */
uint64_t dcrx_cdr3_match_work_bytes(uint64_t m_q, uint64_t text_bytes, uint32_t metric);

/* The primitive: degree and hits of every query against an index, asynchronously on `hip_stream`, the queries' arrays in
 * device memory of the device the index was built on, and `hip_stream` a stream of that device: the call makes that device
 * current for its launches and puts the caller's back before it returns (as dcrx_cdr3_match_run does).  d_class: m_q classes; d_off: m_q + 1 offsets into d_text (text_bytes
 * bytes; a query whose offsets go backwards or leave the text is out of reach).  Writes d_degree (m_q) and d_hit_off
 * (m_q + 1: the exclusive sum of the degrees in rank order).  *d_hit_need (device, uint64) always receives the entries the
 * hits take (= d_hit_off[m_q]); d_hit (hit_cap entries) is written when the need fits hit_cap and is never written past
 * otherwise (an entry beyond hit_cap is dropped), so a caller that finds *d_hit_need > hit_cap calls again with a larger one
 * (d_hit may be NULL with hit_cap 0 to size it).
 * The steps: the queries are prepared as the network prepares its nodes (keys, a stable radix sort of (key, rank), the
 * packed strings gathered in sorted order, presence masks under Levenshtein); then cdr3_walk_kernel (Bipartite): a block holds 256
 * sorted queries in registers, finds the first target at or above its first query's bucket by a binary search over the
 * index's sorted keys, and stages the targets from there in LDS tiles of 256 until the staged bucket passes its last query's
 * bucket; a wave skips a tile that holds none of its buckets; the targets of a bucket are in rank order, so a query's hits
 * come out ascending with no atomics.  The pair test is the network's (csrc/dcrx_cdr3net_core.h).  A degree pass, an
 * exclusive sum, and a write pass that repeats the walk.  Under DCRX_CDR3NET_LEVENSHTEIN with D = 0 the Hamming walk runs.
 * d_work: dcrx_cdr3_match_work_bytes(m_q, text_bytes, metric) bytes, 256-byte aligned; a smaller one is DCRX_E_INVALID, not
 * a launch.  m_q == 0, and an index of 0 targets, launch no kernel (the outputs are zeroed on the stream). */
int dcrx_cdr3_match_device(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off,
                           const char *d_text, uint64_t text_bytes, uint32_t distance, uint32_t metric, uint32_t *d_degree,
                           uint64_t *d_hit_off, uint32_t *d_hit, uint64_t hit_cap, uint64_t *d_hit_need, void *d_work,
                           uint64_t work_bytes, void *hip_stream);

/* The whole step on host arrays, synchronous on the current device, run ONCE whatever is exported afterwards: checks the
 * arguments (all of the contract's refusals, before any device call), uploads the queries, runs the primitive's degree half,
 * allocates exactly the hits it sized (DCRX_E_NOMEM when it cannot) and fills them, then cdr3match_totals_kernel — a lane
 * per query over its CSR row — adds every hit onto its target's t_queries and t_weight by atomics whose results are not
 * read.  *match_out: the result, to be released with dcrx_cdr3_match_destroy (NULL on an error).  m_q == 0, and an index of
 * 0 targets, are answered without a launch. */
int dcrx_cdr3_match_run(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *cls, const uint64_t *off,
                        const char *text, const uint64_t *weight, uint32_t distance, uint32_t metric,
                        dcrx_cdr3_match_t **match_out);
void dcrx_cdr3_match_destroy(dcrx_cdr3_match_t *match);
/* Sizes (queries, targets, hits) and statistics; any pointer may be NULL. */
int dcrx_cdr3_match_info(const dcrx_cdr3_match_t *match, uint64_t *queries, uint64_t *targets, uint64_t *hits,
                         dcrx_cdr3_match_stats_t *stats);
/* Into the caller's arrays, any of which may be NULL: degree (queries), hit_off (queries + 1), hit (hits), t_queries and
 * t_weight (targets each). */
int dcrx_cdr3_match_export(const dcrx_cdr3_match_t *match, uint32_t *degree, uint64_t *hit_off, uint32_t *hit,
                           uint32_t *t_queries, uint64_t *t_weight);

/* The `.cdr3_matches.tsv` text of a CSR of hits in one pass: the header "clonotype v_call j_call junction_aa duplicate_count
 * target distance" followed by a tab and db_header (db_header_bytes bytes: the database's column names, as the caller
 * wants them shown), then one line per hit ordered by (query, target): the query's rank, the calls of v_idx[i] / j_idx[i]
 * (calls: one text, n + 1 offsets), its string and weight, the target's rank, the distance of the two strings under `metric`,
 * computed here on the host (as dcrx_format_cdr3_edges_metric computes it), a tab and the target's line db_lines[db_line_off[j]
 * .. db_line_off[j + 1]) verbatim.  Returns the bytes the text takes; writes it when out != NULL and it fits out_cap.
 * DCRX_E_INVALID for a hit outside the targets, offsets that go backwards, a gene outside its table, a metric that does
 * not exist or, under DCRX_CDR3NET_HAMMING, a hit between strings of two lengths.  Host only. */
int64_t dcrx_format_cdr3_matches(uint64_t m_q, const uint64_t *hit_off, const uint32_t *hit, const uint32_t *v_idx,
                                 const uint32_t *j_idx, uint32_t n_v, const char *v_calls, const uint32_t *v_call_off,
                                 uint32_t n_j, const char *j_calls, const uint32_t *j_call_off, const uint64_t *q_off,
                                 const char *q_text, const uint64_t *weight, uint64_t m_t, const uint64_t *t_off,
                                 const char *t_text, const char *db_header, uint64_t db_header_bytes,
                                 const uint64_t *db_line_off, const char *db_lines, uint32_t metric, char *out,
                                 uint64_t out_cap);

/* ---- match, weighted (`match --cdr3-metric weighted`): the same question under a weighted, TCRdist-style distance with a
 * radius — a conservative substitution costs little, a radical one a lot, a length difference is one gap with a price, and
 * the conserved ends of the CDR3 do not count.  The reference has no counterpart: the contract below is this library's own.
 * The entries only ADD to ABI 5; the entries above keep their signatures and behaviour, and go on refusing metric 2 ----
 *
 * A cost, dcrx_cdr3_cost_t: sub[x][y] the price of letter x against letter y, a letter's index being byte & 31 ('A' 1 ..
 *   'Z' 26; rows and columns 0 and 27 .. 31 are never read); gap, the price of one gapped position, 1 .. 255; ntrim and ctrim,
 *   0 .. 16 each: the first ntrim and the last ctrim positions of the SHORTER string are not counted.  sub is symmetric and
 *   zero on its diagonal over 1 .. 26.  A radius R, 0 .. 65535.  Anything else (an asymmetric entry, a non-zero diagonal,
 *   gap 0 or above 255, a trim above 16, a radius above 65535) is DCRX_E_INVALID, refused on the host before any device call.
 * In reach: the network's rule, 1 <= len <= DCRX_CDR3NET_MAX_LEN (32), and under this metric every byte in 'A' .. 'Z'.  A
 *   node with any other byte (lower case, '*', '_', 0x00, 0x80 and above) takes part in no hit.  The statistics'
 *   *_out_of_reach count the network's rule alone, as under the other metrics; the stage counts the non-letter nodes.
 * The distance of a (la bytes) and b (lb >= la bytes; swapped otherwise), d = lb - la: the gap is ONE block of d positions
 *   put into a behind its first p residues, so a[i] stands against b[i] for i < p and against b[i + d] for i >= p; position i
 *   of a is counted when ntrim <= i < la - ctrim; dist(a, b) = d * gap + min over p in 0 .. la of the sum over the counted i
 *   of sub[a[i]][the byte of b it stands against].  With d = 0 there is no gap and no minimum; with la <= ntrim + ctrim
 *   nothing is counted and dist = d * gap.  (Every p below ntrim costs what p = ntrim costs and every p above la - ctrim what
 *   p = la - ctrim costs; moving the gap from p to p + 1 changes the sum by sub[a[p]][b[p]] - sub[a[p]][b[p + d]].)
 * Hit: (i, j) both in reach, c_i == c_j, dist <= R.  The same bytes on both sides are a hit; two strings that differ in
 *   uncounted positions alone are at distance 0.
 * Output: as dcrx_cdr3_match_run, and hit_dist: per hit the distance the device computed (uint32).  Everything is a function
 *   of the input alone.  m_q, m_t < 2^30 and the weight sum below 2^64, as above. */
#define DCRX_CDR3NET_WEIGHTED 2
typedef struct dcrx_cdr3_cost {
  uint8_t sub[32][32];
  uint32_t gap;
  uint32_t ntrim;
  uint32_t ctrim;
} dcrx_cdr3_cost_t;

/* Bytes of device work space dcrx_cdr3_match_weighted_device needs for m_q queries; 0 for m_q >= 2^30. */
uint64_t dcrx_cdr3_match_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes);

/* The primitive under the weighted metric, with the arguments, the hit_cap / d_hit_need rules and the work-space rules of
 * dcrx_cdr3_match_device (one and the same index serves all three metrics).  `cost` is a HOST pointer: the call checks it
 * and copies it (it travels to the kernels as a launch argument), so the caller may release it on return.  d_hit_dist
 * (hit_cap entries, device) receives every written hit's distance beside d_hit; it may be NULL.
 * The steps: keys, the stable sort by class and the gather of the queries as under Levenshtein (no presence masks: a
 * substitution may cost anything from 0 to 255, so they filter nothing), then cdr3_walk_kernel with the Weighted pair test: the Levenshtein walk's
 * blocks, tiles and wave skip over the index's class-order arrays; the block stages the 1 KB cost table in LDS once; the
 * lane that stages a target tests it for letters and marks the staged key (length 0) so that no lane tests it; a lane
 * tests the class, then the length window |la - lb| * gap <= R, then weighted_within (csrc/dcrx_cdr3w_core.h), pair by pair
 * as it meets them.  A degree pass, an exclusive sum, and a write pass that stores rank and distance. */
int dcrx_cdr3_match_weighted_device(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *d_class,
                                    const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                    const dcrx_cdr3_cost_t *cost, uint32_t radius, uint32_t *d_degree, uint64_t *d_hit_off,
                                    uint32_t *d_hit, uint32_t *d_hit_dist, uint64_t hit_cap, uint64_t *d_hit_need,
                                    void *d_work, uint64_t work_bytes, void *hip_stream);

/* dcrx_cdr3_match_run under the weighted metric: the same handle (dcrx_cdr3_match_info, _export and _destroy serve it),
 * which also keeps the hits' distances. */
int dcrx_cdr3_match_weighted_run(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *cls, const uint64_t *off,
                                 const char *text, const uint64_t *weight, const dcrx_cdr3_cost_t *cost, uint32_t radius,
                                 dcrx_cdr3_match_t **match_out);
/* The distances of a weighted handle's hits, in the order of `hit` (hits entries; may be NULL).  DCRX_E_INVALID for a handle
 * of dcrx_cdr3_match_run, which has none. */
int dcrx_cdr3_match_export_dist(const dcrx_cdr3_match_t *match, uint32_t *hit_dist);

/* dcrx_format_cdr3_matches with the weighted distance in the distance column, computed here on the host from the two
 * strings as the literal minimum over every p in 0 .. la (not the device's one-pass form).  DCRX_E_INVALID in addition for a
 * cost the contract refuses, and for a hit between strings out of reach or with a byte outside 'A' .. 'Z'. */
int64_t dcrx_format_cdr3_matches_weighted(uint64_t m_q, const uint64_t *hit_off, const uint32_t *hit, const uint32_t *v_idx,
                                          const uint32_t *j_idx, uint32_t n_v, const char *v_calls,
                                          const uint32_t *v_call_off, uint32_t n_j, const char *j_calls,
                                          const uint32_t *j_call_off, const uint64_t *q_off, const char *q_text,
                                          const uint64_t *weight, uint64_t m_t, const uint64_t *t_off, const char *t_text,
                                          const char *db_header, uint64_t db_header_bytes, const uint64_t *db_line_off,
                                          const char *db_lines, const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap);

/* ---- profile, weighted (`metaclonotypes`): per query, HOW MANY targets lie at which weighted distance — a histogram over a
 * ladder of radii from ONE walk, where "match, weighted" answers one radius.  The reference has no counterpart: the contract
 * below is this library's own.  The entries only ADD to ABI 5; the entries above keep their signatures and behaviour ----
 *
 * Input: a dcrx_cdr3_index_t (the targets), queries as dcrx_cdr3_match_weighted_device takes them (class, string; no weight), a
 *   cost (dcrx_cdr3_cost_t), a `step` of 1 .. 65535 and `bins` of 1 .. 32.  R = step * (bins - 1) is the ladder's top and is at
 *   most 65535.
 * Reach, letters-only, classes and the distance are exactly those of "match, weighted": a node takes part when it has 1 .. 32
 *   bytes, all 'A' .. 'Z'.
 * Output: profile[i * bins + b] (uint32) = the number of targets j for which query i and target j both take part, c_i == c_j
 *   and ceil(dist(i, j) / step) == b.  So bin 0 holds the targets at distance 0 and bin b those with
 *   (b - 1) * step < dist <= b * step; a target beyond R is in no bin.  The cells are NOT cumulative: the caller takes prefix
 *   sums, and for every i and b the sum of profile[i][0 .. b] is the degree[i] dcrx_cdr3_match_weighted_run gives at radius
 *   b * step.  A query that takes no part (out of reach, or with a non-letter) has a row of zeros.  Every one of the m_q * bins
 *   cells is written by the call: the caller's buffer need not be cleared.  Everything is an integer and a function of the input
 *   alone; nothing depends on launch shape or on the order of arrival.
 * Refused on the host before any launch with DCRX_E_INVALID: what "match, weighted" refuses of a cost; step 0 (or above
 *   65535); bins 0 or above 32; step * (bins - 1) > 65535; a null profile with m_q > 0; a work space that is short or not
 *   256-byte aligned.  m_q = 0 is valid (nothing is written), and so is an index of 0 targets (all zeros).  m_q < 2^30
 *   (DCRX_E_UNSUPPORTED beyond). */
typedef struct dcrx_cdr3_profile_stats {
  uint64_t queries;
  uint64_t targets;
  uint64_t queries_out_of_reach;    /* the network's rule: the length alone */
  uint64_t queries_not_letters;     /* in that reach, with a byte outside 'A' .. 'Z' */
  uint64_t targets_out_of_reach;    /* the index's count (length alone) */
  uint64_t cells_sum;               /* the sum of all cells: the (query, target) pairs within R */
  uint64_t queries_nonzero;         /* queries with a non-zero row */
} dcrx_cdr3_profile_stats_t;

/* Bytes of device work space dcrx_cdr3_profile_weighted_device needs for m_q queries (their sorted keys, ranks and packed
 * strings and the sort's scratch: the histogram itself lives in LDS, so `bins` does not enter the size); 0 for m_q >= 2^30 and
 * for bins outside 1 .. 32.  Answered on the host. */
uint64_t dcrx_cdr3_profile_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes, uint32_t bins);

/* The primitive, asynchronous on `hip_stream`, with the device arrays, the device rule (the index's device is made current
 * for the launches) and the work-space rules of dcrx_cdr3_match_weighted_device; `cost` is a HOST pointer, checked and
 * copied.  d_profile: m_q * bins dwords of device memory.
 * The steps: keys, the stable sort by class and the gather without masks, as the weighted match prepares its queries; then
 * cdr3_walk_kernel<false, Bipartite, Weighted, Profile>: the weighted match's blocks of 256 queries in registers, LDS tiles of
 * 256 targets, wave skip and staged cost table, with the pair test at radius R (it returns R + 1 for anything beyond and keeps
 * its early exits).  What happens to a tested pair is the sink's: d <= R adds one to the lane's counter of bin
 * ceil(d / step) (csrc/dcrx_cdr3profile_core.h: bin_of, a true division).  A lane's counters are a column of its own in
 * dynamic LDS, hist[b * 256 + lane] — bins KB a block, conflict-free across lanes, one LDS add without a returned value per
 * hit — zeroed in front of the walk and read out behind it into row Q.idx[s]; lanes behind the table write nothing.  One
 * launch of the walk whatever `bins` is.  An index of 0 targets zeroes the profile on the stream without a kernel. */
int dcrx_cdr3_profile_weighted_device(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *d_class,
                                      const uint64_t *d_off, const char *d_text, uint64_t text_bytes,
                                      const dcrx_cdr3_cost_t *cost, uint32_t step, uint32_t bins, uint32_t *d_profile,
                                      void *d_work, uint64_t work_bytes, void *hip_stream);

/* The whole step on host arrays, synchronous on the index's device: checks the arguments (all of the contract's refusals,
 * offsets that go backwards and null arrays too, before any device call), uploads the queries into ONE allocation that also
 * holds the profile and the work space, runs the primitive's steps and copies the profile (m_q * bins dwords) back.  `stats`
 * may be NULL.  m_q == 0, and an index of 0 targets, are answered without a launch. */
int dcrx_cdr3_profile_weighted(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *cls, const uint64_t *off,
                               const char *text, const dcrx_cdr3_cost_t *cost, uint32_t step, uint32_t bins,
                               uint32_t *profile, dcrx_cdr3_profile_stats_t *stats);

/* ---- tally, weighted (`tabulate`): per TARGET, how many queries — and how much of their weight — lie within that target's OWN
 * radius: meta-clonotypes (centroid, class, radius) counted in a bulk sample.  "match, weighted" takes one radius and lists
 * pairs; this takes a radius per target and leaves totals only: no hit list, no second pass, memory linear in the tables.  The
 * reference has no counterpart: the contract below is this library's own.  The entries only ADD to ABI 5; the entries above
 * keep their signatures and behaviour ----
 *
 * Input: a dcrx_cdr3_index_t (the targets); per target, by rank, a radius r_j (uint32): 0 .. 65535, or DCRX_CDR3_NO_RADIUS,
 *   which means that the target takes part in nothing; queries as dcrx_cdr3_match_weighted_device takes them (class, string)
 *   with a weight w_i (uint64); a cost (dcrx_cdr3_cost_t).
 * Reach, letters-only, classes and the distance are exactly those of "match, weighted".
 * Hit: (i, j) is a hit when both take part, c_i == c_j, r_j is a radius and dist(i, j) <= r_j.
 * Output: t_count[j] (uint32) = the queries that hit target j; t_weight[j] (uint64) = the sum of their weights; q_degree[i]
 *   (uint32) = the targets query i hits (with it the caller counts the queries inside ANY target without counting one twice).
 *   Every one of the m_t + m_t + m_q cells is written by the call: the caller's buffers need not be cleared.  Everything is an
 *   integer and a function of the input alone: integer adds, and atomics whose results are not read.  With every r_j = R the
 *   three arrays are t_queries, t_weight and degree of dcrx_cdr3_match_weighted_run at R.
 * Refused on the host before any launch with DCRX_E_INVALID: what "match, weighted" refuses of a cost; a null output with a
 *   non-zero size; a work space that is short or not 256-byte aligned; in the host entry a radius in 65536 .. 0xFFFFFFFE and
 *   offsets that go backwards.  A weight sum at or above 2^64 is DCRX_E_UNSUPPORTED (the host entry sees it), and so is
 *   m_q >= 2^30 (an index holds fewer than 2^30 targets).  m_q = 0 zeroes the target arrays on the stream without a kernel,
 *   and an index of 0 targets zeroes q_degree the same way; neither looks at the work space. */
#define DCRX_CDR3_NO_RADIUS 0xFFFFFFFFu

typedef struct dcrx_cdr3_tally_stats {
  uint64_t queries;
  uint64_t targets;
  uint64_t queries_out_of_reach;    /* the network's rule: the length alone */
  uint64_t queries_not_letters;     /* in that reach, with a byte outside 'A' .. 'Z' */
  uint64_t targets_out_of_reach;    /* the index's count (length alone) */
  uint64_t targets_without_radius;  /* r_j == DCRX_CDR3_NO_RADIUS */
  uint64_t hits;                    /* the sum of q_degree */
  uint64_t queries_hit;             /* queries with q_degree > 0 */
  uint64_t queries_hit_weight;      /* the sum of their weights */
  uint64_t targets_hit;             /* targets with t_count > 0 */
} dcrx_cdr3_tally_stats_t;

/* Bytes of device work space dcrx_cdr3_tally_weighted_device needs for m_q queries against an index of m_t targets (the
 * queries' sorted keys, ranks and packed strings, the sort's scratch, and a count and a weight accumulator per target); 0 for
 * m_q >= 2^30 or m_t >= 2^30.  Answered on the host. */
uint64_t dcrx_cdr3_tally_weighted_work_bytes(uint64_t m_q, uint64_t text_bytes, uint64_t m_t);

/* The primitive, asynchronous on `hip_stream`, with the device arrays, the device rule (the index's device is made current
 * for the launches) and the work-space rules of dcrx_cdr3_match_weighted_device; `cost` is a HOST pointer, checked and
 * copied.  d_weight: m_q uint64; d_radius: m_t uint32 by rank; d_t_count, d_t_weight: m_t; d_q_degree: m_q — all device memory.
 * The host cannot see the radii here: a value above 65535 is treated on the device as DCRX_CDR3_NO_RADIUS.
 * The steps: keys, the stable sort by class and the gather without masks, as the weighted match prepares its queries; the two
 * accumulators zeroed; then cdr3_walk_kernel<false, Bipartite, WeightedPer, Tally>: the weighted match's walk, where the lane
 * that stages a target also stages its radius (a gather by rank; the index is untouched) and a target without one gets a key
 * of length 0, as one with a non-letter does; the length window and the pair test run at the staged target's own radius.  A
 * hit adds one and the lane's weight to the staged target's two cells in LDS; per tile, lane k adds target k's non-zero cells
 * onto the accumulators in the work space, which are indexed by the index's SORTED position, so that a wave's adds touch
 * contiguous addresses: at most two global atomics per (block, staged target).  cdr3_tally_scatter_kernel then writes every
 * target's two cells by rank.  q_degree[i] is written by the lane that holds query i. */
int dcrx_cdr3_tally_weighted_device(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *d_class, const uint64_t *d_off,
                                    const char *d_text, uint64_t text_bytes, const uint64_t *d_weight,
                                    const dcrx_cdr3_cost_t *cost, const uint32_t *d_radius, uint32_t *d_t_count,
                                    uint64_t *d_t_weight, uint32_t *d_q_degree, void *d_work, uint64_t work_bytes,
                                    void *hip_stream);

/* The whole step on host arrays, synchronous on the index's device: checks the arguments (all of the contract's refusals and
 * null arrays, before any device call), uploads the queries and the radii into ONE allocation that also holds the outputs and
 * the work space, runs the primitive's steps and copies the three arrays back.  `stats` may be NULL.  m_q == 0, and an index
 * of 0 targets, are answered without a launch and without a device call. */
int dcrx_cdr3_tally_weighted(const dcrx_cdr3_index_t *index, uint64_t m_q, const uint32_t *cls, const uint64_t *off,
                             const char *text, const uint64_t *weight, const dcrx_cdr3_cost_t *cost, const uint32_t *radius,
                             uint32_t *t_count, uint64_t *t_weight, uint32_t *q_degree, dcrx_cdr3_tally_stats_t *stats);

/* ---- association (`associate`): the label-permutation null of exact tests over a feature by sample table — every feature
 * scored again under every relabeling of the samples, on the GPU.  This layer knows nothing about tests, genes or files: the
 * caller hands it a table of RANKS of p-values and gets integers back.  The reference has no counterpart: the contract below is
 * this library's own.  The entries only ADD to ABI 5 ----
 *
 * Input: N samples, 2 <= N <= DCRX_ASSOC_MAX_SAMPLES (64); a case mask C (uint64, no bit at or above N), n1 = popcount(C),
 *   1 <= n1 <= N - 1; F features, F < 2^30, each a presence mask M_f (uint64, no bit at or above N) and a multiplicity w_f
 *   (uint32; 0: the feature takes part in nothing), the sum of the w_f below 2^32; a rank table rank[(N + 1) * (N + 1)] of
 *   uint16 indexed m * (N + 1) + k, smaller = more extreme: a cell (m, k) is feasible when max(0, m - (N - n1)) <= k <=
 *   min(m, n1), feasible cells hold 0 .. n_ranks - 1 and the other cells are never read; n_ranks <= (N + 1)^2; tail_ranks in
 *   0 .. n_ranks; P permutations, 0 <= P <= DCRX_ASSOC_MAX_PERMUTATIONS (2^20); one 64-bit seed.
 * Relabeling p (p = 0 .. P - 1): L_p is the set of the n1 samples s in 0 .. N - 1 with the smallest key(seed, p, s), key the
 *   function of "downsample" with p in the sample's place and s in the read's.  The keys of one p are pairwise distinct, as
 *   there: no tie rule.
 * Score: m_f = popcount(M_f); r_p(f) = rank[m_f][popcount(M_f & L_p)]; the observed score r(f) = rank[m_f][popcount(M_f & C)].
 *   Every index reached is a feasible cell, because popcount(L_p) = n1.
 * Output, every cell written by the call (the caller's buffers need not be cleared), integers only — integer adds, and atomics
 *   whose results are not read; nothing depends on launch shape or order of arrival:
 *     obs_rank[f] (uint32) = r(f), also where w_f = 0;   labels[p] (uint64) = L_p;
 *     perm_min[p] (uint32) = the minimum over f with w_f > 0 of r_p(f), n_ranks when there is no such f;
 *     tail[r] (uint64), r < tail_ranks, = the sum over p and f of w_f [r_p(f) = r]  (below 2^52 by the limits above).
 * DCRX_E_INVALID: N outside 2 .. 64; C with a bit at or above N, or n1 of 0 or N; n_ranks of 0 or above (N + 1)^2; tail_ranks
 *   above n_ranks; a null array with a non-zero size (the table always has one); in the host entry a mask with a bit at or
 *   above N and a feasible cell at or above n_ranks.  DCRX_E_UNSUPPORTED: F >= 2^30; P > 2^20; in the host entry a multiplicity
 *   sum of 2^32 or more.  The scalars are judged in this order, before the arrays.
 * Which test the ranks stand for (one- or two-sided, Fisher's or another), and so whether the table is monotone in k, is the
 * caller's business: nothing here assumes it. */
#define DCRX_ASSOC_MAX_SAMPLES 64
#define DCRX_ASSOC_MAX_PERMUTATIONS (1u << 20)

typedef struct dcrx_assoc_stats {
  uint64_t features;           /* F */
  uint64_t features_weighted;  /* those with w_f > 0 */
  uint64_t weight;             /* the sum of the w_f */
  uint64_t permutations;       /* P */
  uint64_t tail_total;         /* the sum of tail[] */
  uint64_t min_perm_rank;      /* the smallest perm_min (n_ranks where there is none) */
} dcrx_assoc_stats_t;

/* The primitive, asynchronous on `hip_stream`, all arrays in device memory: d_mask, d_mult and d_obs_rank F entries, d_rank
 * (N + 1)^2, d_labels and d_perm_min P, d_tail tail_ranks.  Nothing is copied back, nothing waits, nothing is allocated: THE
 * ENTRY TAKES NO WORK SPACE (the relabelings live in d_labels, everything else in registers and LDS).
 * The steps: assoc_prepare_kernel, a lane per index, sets tail to 0 and writes obs_rank; assoc_labels_kernel, a lane per
 * relabeling in blocks of 64, writes the relabeling's N keys once into the lane's own column of LDS, finds L_p by N^2 compares
 * from there (no array of keys in registers) and sets perm_min to n_ranks; assoc_permute_kernel runs on a grid of (slices of 1024 features) x
 * (tiles of 1024 relabelings): a block keeps the rank table (uint16) and its own tail cells in LDS, a lane four relabelings and
 * their running minima in registers; a feature's mask, row and multiplicity are the same for the whole wave; per pair an AND,
 * a popcount, one LDS read, a min and a compare, and only where the rank is below tail_ranks an LDS add of w_f whose result is
 * not read.  A block's tail cells are 64 bits wide — a block adds at most 1024 * 1024 multiplicities below 2^32 onto one cell,
 * below 2^52 — so nothing is flushed before the block's end: one global atomic min per (lane, relabeling), one global 64-bit
 * atomic add per non-zero tail cell.
 * What only the device can see: every mask is ANDed with the N-bit mask, and a rank adds to tail only where it is below
 * tail_ranks, so nothing is read or written outside the arrays, whatever they hold. */
int dcrx_assoc_permute_device(uint32_t n_samples, uint64_t case_mask, uint64_t n_features, const uint64_t *d_mask,
                              const uint32_t *d_mult, const uint16_t *d_rank, uint32_t n_ranks, uint32_t tail_ranks,
                              uint32_t permutations, uint64_t seed, uint32_t *d_obs_rank, uint64_t *d_labels,
                              uint32_t *d_perm_min, uint64_t *d_tail, void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays of the same shapes: every refusal above before any device
 * call, ONE allocation, the uploads, the primitive on the null stream, the four arrays copied back.  `stats_out` may be NULL.
 * F == 0 or P == 0 is answered on the host and touches no device: obs_rank and labels are computed here, perm_min is n_ranks,
 * tail is 0. */
int dcrx_assoc_permute(uint32_t n_samples, uint64_t case_mask, uint64_t n_features, const uint64_t *mask, const uint32_t *mult,
                       const uint16_t *rank, uint32_t n_ranks, uint32_t tail_ranks, uint32_t permutations, uint64_t seed,
                       uint32_t *obs_rank_out, uint64_t *labels_out, uint32_t *perm_min_out, uint64_t *tail_out,
                       dcrx_assoc_stats_t *stats_out);

/* ---- association, wide (`associate` on cohorts of 65 to 1024 samples): the contract of "association" above with a presence
 * pattern and a relabeling of W words in place of one, and ranks of 32 bits.  The narrow entries, their limit of 64 samples and
 * their behaviour stay as they are.  The entries only ADD to ABI 5 ----
 *
 * Samples and words: N samples, 2 <= N <= DCRX_ASSOC_WIDE_MAX_SAMPLES (1024), in W = ceil(N / 64) words of uint64: sample s is
 *   bit s & 63 of word s >> 6.  N <= 64 is served with W = 1 and gives what the narrow layer gives.
 * Input: a case mask C, a pointer to W words IN HOST MEMORY in both entries (read during the call; no bit at or above N),
 *   n1 = its popcount, 1 <= n1 <= N - 1; F features, F < 2^30: `mask` is F x W uint64, row-major, feature f's words at
 *   mask[f W .. f W + W - 1], no bit at or above N; `mult` as above (uint32; 0: the feature takes part in nothing), the sum
 *   below 2^32; a rank table rank[(N + 1) * (N + 1)] of UINT32 indexed m * (N + 1) + k (a balanced cohort of 1024 has 131 074
 *   distinct one-sided p-values: sixteen bits do not hold them), feasible cells hold 0 .. n_ranks - 1, the others are never
 *   read; n_ranks <= (N + 1)^2; tail_ranks in 0 .. n_ranks; P permutations, 0 <= P <= DCRX_ASSOC_MAX_PERMUTATIONS; one seed.
 * Relabeling p: L_p is the n1 samples with the smallest key(seed, p, s) — the key of "association", so for N <= 64 the
 *   relabelings are the narrow layer's, bit for bit.
 * Score: m_f = the sum over the words of popcount(M_f,w); k = the sum over the words of popcount(M_f,w & L_p,w);
 *   r_p(f) = rank[m_f][k]; the observed score r(f) uses C in L_p's place.
 * Output, every cell written by the call, integers only — integer adds, and atomics whose results are not read; nothing depends
 *   on launch shape, on order of arrival or on the ORDER OF THE FEATURES (features may come in any order of popcount: only the
 *   speed depends on it, fastest in ascending or descending popcount):
 *     obs_rank[f] (uint32) = r(f), also where w_f = 0;   labels[p W + w] (uint64) = word w of L_p;
 *     perm_min[p] (uint32) = the minimum over f with w_f > 0 of r_p(f), n_ranks when there is no such f;
 *     tail[r] (uint64), r < tail_ranks, = the sum over p and f of w_f [r_p(f) = r]  (below 2^52).
 * Refusals, in this order.  The scalars: DCRX_E_INVALID for N outside 2 .. 1024, n_ranks of 0 or above (N + 1)^2, tail_ranks
 *   above n_ranks; DCRX_E_UNSUPPORTED for F >= 2^30 and P > 2^20.  Then DCRX_E_INVALID for a null array with a non-zero size
 *   (the case mask and the table always have one).  Then the case mask: DCRX_E_INVALID for n1 of 0 or N.  What the host entry
 *   alone can see it alone refuses, in this order: DCRX_E_INVALID for a case-mask bit at or above N (before n1 is judged), for a
 *   feasible cell at or above n_ranks and for a mask bit at or above N; DCRX_E_UNSUPPORTED for a multiplicity sum of 2^32 or
 *   more.  The device entry instead ANDs the last word of the case mask and of every mask with the N-bit remainder, adds to
 *   tail only below tail_ranks and indexes a row of the table only with k <= m <= N: nothing outside the arrays is read or
 *   written, whatever the arrays hold. */
#define DCRX_ASSOC_WIDE_MAX_SAMPLES 1024

/* The primitive, asynchronous on `hip_stream`: d_mask F x W, d_mult and d_obs_rank F, d_rank (N + 1)^2 (uint32), d_labels
 * P x W, d_perm_min P, d_tail tail_ranks, all in device memory; case_mask W words in host memory, copied into the launches'
 * arguments before the call returns.  Nothing is copied back, nothing waits, nothing is allocated: THE ENTRY TAKES NO WORK
 * SPACE.
 * The steps: assoc_wide_prepare_kernel, a lane per index, sets tail to 0 and writes obs_rank; assoc_wide_labels_kernel, a block
 * per relabeling, stages the N keys once in LDS (8 KB at most), has every lane count the keys smaller than its samples' from
 * broadcast reads, assembles each word with a ballot and sets perm_min to n_ranks; assoc_wide_permute_kernel<W>, one
 * instance per W = 1 .. 16 with W a constant in it, runs on a grid of (slices of 1024 features) x (tiles of 1024, 512 or 256 relabelings at up to 4, 8 or 16 words): a
 * lane keeps 4, 2 or 1 relabelings and their minima in registers, the block walks its slice in runs of equal popcount m with
 * the row of m (N + 1 uint32) and one 64-bit cell per k in LDS, 12 KB at most whatever tail_ranks is; on a change of m it adds
 * the non-zero cells to tail[row[k]] where row[k] < tail_ranks and stages the next row.  A feature's words and multiplicity are
 * the same for the whole block; a word that is 0 is skipped: branched over up to 8 words, and from 9 words on, at one relabeling
 * a lane, left by the compiler as two popcounts and a select (profiles/assoc_wide/resource_usage.md). */
int dcrx_assoc_permute_wide_device(uint32_t n_samples, const uint64_t *case_mask, uint64_t n_features, const uint64_t *d_mask,
                                   const uint32_t *d_mult, const uint32_t *d_rank, uint32_t n_ranks, uint32_t tail_ranks,
                                   uint32_t permutations, uint64_t seed, uint32_t *d_obs_rank, uint64_t *d_labels,
                                   uint32_t *d_perm_min, uint64_t *d_tail, void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays of the same shapes: every refusal above before any device
 * call, ONE allocation, the uploads, the primitive on the null stream, the four arrays copied back.  `stats_out` may be NULL.
 * F == 0 or P == 0 is answered on the host and touches no device. */
int dcrx_assoc_permute_wide(uint32_t n_samples, const uint64_t *case_mask, uint64_t n_features, const uint64_t *mask,
                            const uint32_t *mult, const uint32_t *rank, uint32_t n_ranks, uint32_t tail_ranks,
                            uint32_t permutations, uint64_t seed, uint32_t *obs_rank_out, uint64_t *labels_out,
                            uint32_t *perm_min_out, uint64_t *tail_out, dcrx_assoc_stats_t *stats_out);

/* ---- association, rank-sum (`associate --test rank-sum`): the label-permutation null of a Wilcoxon / Mann-Whitney rank sum per
 * feature — a test on ABUNDANCE, beside the presence tests of "association" — with what Westfall and Young's single-step max-T
 * needs.  This layer knows nothing about ranks, ties, depths or files: the caller hands it small integer SCORES per feature and
 * sample, as bit planes, and two integers per feature that standardize a sum of them.  Integers only; every output an exact
 * function of the input.  The narrow and the wide entries stay as they are.  The entries only ADD to ABI 5 ----
 *
 * Input: N samples, 2 <= N <= DCRX_ASSOC_MAX_SAMPLES (64); a case mask C (uint64, no bit at or above N), n1 = popcount(C),
 *   1 <= n1 <= N - 1; an alternative: 0 greater, 1 less, 2 two-sided; F features, F < 2^30; P permutations, 0 <= P <=
 *   DCRX_ASSOC_MAX_PERMUTATIONS (2^20); one 64-bit seed; plane[F][DCRX_ASSOC_RANKSUM_PLANES] (uint64, row-major): bit b of the
 *   score a[f][s], 0 <= a < 128, is bit s of plane[f * 7 + b], no bit at or above N; offset[F], scale[F] and mult[F] (uint32;
 *   mult 0: the feature takes part in perm_max and tail not at all), the sum of the mult below 2^32; edges[E] (uint32),
 *   E <= DCRX_ASSOC_RANKSUM_MAX_EDGES (1024), strictly ascending.
 * Relabeling p (p = 0 .. P - 1): L_p of "association" — the n1 samples with the smallest key(seed, p, s).  For the same N, C and
 *   seed these are the words dcrx_assoc_permute returns.
 * Score of feature f under a labeling L: W = the sum over s in L of a[f][s] = the sum over b of popcount(plane[f][b] & L) << b;
 *   D = N W - offset[f], a signed 64-bit value; u = D (greater), -D (less) or |D| (two-sided), clamped to 0 .. 2^20 - 1;
 *   t = (u * scale[f]) >> DCRX_ASSOC_RANKSUM_SHIFT (20), a uint32 whatever the arrays hold (at most 2^32 - 4097).  The caller
 *   that wants a standardized rank sum hands over a = the doubled mid-rank less its minimum, offset = n1 sum(a) and scale =
 *   min(2^32 - 1, isqrt(2^64 / (N sum(a^2) - sum(a)^2))), 0 where every value is equal: t_p(f) is L_p's score, the observed
 *   score is C's.
 * Output, every cell written by the call (the caller's buffers need not be cleared) — integer adds and maxima, and atomics whose
 *   results are not read; nothing depends on launch shape or order of arrival:
 *     obs_score[f] (uint32) = t under C, also where mult[f] = 0;   labels[p] (uint64) = L_p;
 *     perm_max[p] (uint32) = the maximum over f with mult[f] > 0 of t_p(f), 0 when there is no such f;
 *     exceed[f] (uint32) = #{p : t_p(f) >= obs_score[f]}, for EVERY feature, mult[f] = 0 included;
 *     tail[j] (uint64), j < E, = the sum over p and f of mult[f] [j is the largest index with edges[j] <= t_p(f)]: a pair below
 *       edges[0] falls in no cell (below 2^52 by the limits above).
 * Refusals, in this order.  The scalars, as "association" judges them with the alternative and E in the place of its two rank
 *   counts: DCRX_E_INVALID for N outside 2 .. 64, C with a bit at or above N, n1 of 0 or N, an alternative above 2, E above 1024;
 *   DCRX_E_UNSUPPORTED for F >= 2^30 and P > 2^20.  Then DCRX_E_INVALID for a null array with a non-zero size.  What the host
 *   entry alone can see it alone refuses, in this order: DCRX_E_INVALID for a plane bit at or above N and for edges that are not
 *   strictly ascending, DCRX_E_UNSUPPORTED for a multiplicity sum of 2^32 or more.  The device entry instead ANDs every plane
 *   with the N-bit mask, clamps u, and searches the edges only inside 0 .. E - 1 (what it finds in edges that do not ascend is
 *   some cell of tail, or none): nothing outside the arrays is read or written, whatever they hold. */
#define DCRX_ASSOC_RANKSUM_PLANES 7
#define DCRX_ASSOC_RANKSUM_SHIFT 20
#define DCRX_ASSOC_RANKSUM_MAX_EDGES 1024

typedef struct dcrx_assoc_ranksum_stats {
  uint64_t features;           /* F */
  uint64_t features_weighted;  /* those with mult > 0 */
  uint64_t weight;             /* the sum of the mult */
  uint64_t permutations;       /* P */
  uint64_t tail_total;         /* the sum of tail[] */
  uint64_t max_perm_score;     /* the largest perm_max (0 where there is none) */
} dcrx_assoc_ranksum_stats_t;

/* The primitive, asynchronous on `hip_stream`, all arrays in device memory: d_plane 7 F words, d_offset, d_scale, d_mult,
 * d_obs_score and d_exceed F entries, d_edges and d_tail E, d_labels and d_perm_max P.  Nothing is copied back, nothing waits,
 * nothing is allocated: THE ENTRY TAKES NO WORK SPACE (the relabelings live in d_labels, everything else in registers and LDS).
 * The steps: assoc_ranksum_prepare_kernel, a lane per index, sets tail and exceed to 0 and writes obs_score;
 * assoc_ranksum_labels_kernel, the selection of "association" (the same device function) with perm_max set to 0;
 * assoc_ranksum_permute_kernel on a grid of (slices of 1024 features) x (tiles of 1024 relabelings), 256 lanes, four relabelings
 * and their maxima a lane in registers: a feature's seven plane words, offset, scale, multiplicity and observed score are the same
 * for the whole wave and are asked for four features at a time; a plane word that is 0 is skipped; per pair and non-zero plane an
 * AND, a popcount and a shift-add, then a multiply-subtract, the alternative's side, a 32 x 32 -> 64 multiply, a shift and a
 * max.  exceed: a wave ballot of t >= obs over the lanes that hold a relabeling, counted once a wave, one LDS add per (wave,
 * feature), one global atomic add per non-zero feature of the block.  tail: only where t >= edges[0]; below edges[1] — cell 0,
 * where most pairs of a null fall — a second ballot and one 64-bit LDS add per (wave, feature), above it a binary search of the
 * edges in LDS and a 64-bit LDS add of the multiplicity; one global 64-bit atomic add per non-zero cell of the block.  perm_max:
 * one global atomic max per (lane, relabeling) above 0.  LDS: the tail cells (64 bits, first), the edges and the slice's exceed
 * counters, 16 KB. */
int dcrx_assoc_ranksum_device(uint32_t n_samples, uint64_t case_mask, uint32_t alternative, uint64_t n_features,
                              const uint64_t *d_plane, const uint32_t *d_offset, const uint32_t *d_scale, const uint32_t *d_mult,
                              uint32_t n_edges, const uint32_t *d_edges, uint32_t permutations, uint64_t seed,
                              uint32_t *d_obs_score, uint64_t *d_labels, uint32_t *d_perm_max, uint32_t *d_exceed, uint64_t *d_tail,
                              void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays of the same shapes: every refusal above before any device
 * call, ONE allocation, the uploads, the primitive on the null stream, the five arrays copied back.  `stats_out` may be NULL.
 * F == 0 or P == 0 is answered on the host and touches no device: obs_score and labels are computed here, perm_max, exceed and
 * tail are 0. */
int dcrx_assoc_ranksum(uint32_t n_samples, uint64_t case_mask, uint32_t alternative, uint64_t n_features, const uint64_t *plane,
                       const uint32_t *offset, const uint32_t *scale, const uint32_t *mult, uint32_t n_edges, const uint32_t *edges,
                       uint32_t permutations, uint64_t seed, uint32_t *obs_score_out, uint64_t *labels_out, uint32_t *perm_max_out,
                       uint32_t *exceed_out, uint64_t *tail_out, dcrx_assoc_ranksum_stats_t *stats_out);

/* ---- the CDR3 network, weighted (`--cdr3-network --cdr3-metric weighted`): which clonotypes of ONE table lie within a radius
 * of each other under the weighted distance above, and the clusters they form.  The entries only ADD to ABI 5; the network's
 * *_metric entries keep their signatures and behaviour, and go on refusing metric 2 ----
 *
 * Input: the nodes of dcrx_cdr3_network (class c_i, string s_i, weight w_i; m < 2^30), a cost (dcrx_cdr3_cost_t) and a radius R,
 *   0 .. 65535, with the rules and the DCRX_E_INVALID refusals of "match, weighted" (one routine checks both).
 * In reach: as under "match, weighted", 1 <= len <= 32 and every byte in 'A' .. 'Z'.  A node outside that reach has no
 *   neighbours: degree 0, a cluster of its own, in nobody's row.  stats.out_of_reach keeps the network's meaning: length alone.
 * Edge: i != j, both in reach, c_i == c_j, dist(s_i, s_j) <= R, dist exactly that of "match, weighted".  Equal strings in one
 *   class are linked at distance 0 (two J calls under class v).
 * Output: as dcrx_cdr3_network — degree, the CSR adjacency with every row in ascending rank, cluster_of, the cluster rows by
 *   head ascending, dcrx_cdr3_network_stats_t (edges: the pairs within R) — and per adjacency entry the distance the device
 *   computed.  The adjacency is symmetric and so are its distances; clusters are the connected components (a chain links its
 *   ends).  Everything is a function of the input alone.
 * The steps: keys, the stable sort by class and the run marks by class as under Levenshtein, the gather without presence
 *   masks, then cdr3_walk_kernel<WRITE, Within, Weighted>: the table walked against itself from each block's first class
 *   start, a node never testing its own entry.  Every unordered pair is computed twice, once by the shorter string's lane
 *   (which reads the other string at i and i + d) and once by the longer string's (which shifts its own words down by d bytes). */

/* Bytes of device work space dcrx_cdr3_neighbours_weighted_device needs for m nodes (no presence masks: what
 * dcrx_cdr3net_work_bytes gives); 0 for m >= 2^30. */
uint64_t dcrx_cdr3net_weighted_work_bytes(uint64_t m, uint64_t text_bytes);

/* The primitive: dcrx_cdr3_neighbours_metric_device's arguments, adj_cap / d_adj_need rules and null, alignment and
 * short-work-space refusals, with (cost, radius) in place of (distance, metric).  `cost` is a HOST pointer: the call checks it
 * and copies it (it travels to the kernels as a launch argument).  d_adj_dist (adj_cap entries, device) receives every written
 * neighbour's distance beside d_adj; it may be NULL.  Asynchronous on hip_stream. */
int dcrx_cdr3_neighbours_weighted_device(uint64_t m, const uint32_t *d_class, const uint64_t *d_off, const char *d_text,
                                         uint64_t text_bytes, const dcrx_cdr3_cost_t *cost, uint32_t radius, uint32_t *d_degree,
                                         uint64_t *d_adj_off, uint32_t *d_adj, uint32_t *d_adj_dist, uint64_t adj_cap,
                                         uint64_t *d_adj_need, void *d_work, uint64_t work_bytes, void *hip_stream);

/* dcrx_cdr3_network_metric's arguments, rules and errors with (cost, radius) in place of (distance, metric), and adj_dist_out
 * (adj_cap entries; may be NULL) beside adj_out: written wherever adj_out is. */
int64_t dcrx_cdr3_network_weighted(uint64_t m, const uint32_t *cls, const uint64_t *off, const char *text, const uint64_t *weight,
                                   const dcrx_cdr3_cost_t *cost, uint32_t radius, uint32_t *degree_out, uint32_t *cluster_of_out,
                                   uint32_t *head_out, uint32_t *n_nodes_out, uint64_t *weight_out, uint64_t *adj_off_out,
                                   uint32_t *adj_out, uint32_t *adj_dist_out, uint64_t adj_cap, uint64_t *adj_need_out,
                                   dcrx_cdr3_network_stats_t *stats_out);

/* dcrx_format_cdr3_edges with the weighted distance in the distance column, computed here on the host as the literal minimum
 * over every p in 0 .. la (dcrx_format_cdr3_matches_weighted's routine, not the device's one-pass form).  DCRX_E_INVALID in
 * addition for a cost the contract refuses and for an edge between strings out of reach or with a byte outside 'A' .. 'Z'. */
int64_t dcrx_format_cdr3_edges_weighted(uint64_t m, const uint64_t *adj_off, const uint32_t *adj, const uint64_t *off,
                                        const char *text, const dcrx_cdr3_cost_t *cost, char *out, uint64_t out_cap);

/* ---- motifs (`motifs`): which short motifs (2-, 3- and 4-mers in the middle of a CDR3) a sample's CDR3s hold more often than
 * as many CDR3s drawn from a background do, on the GPU.  The reference has no counterpart: the contract below is this library's
 * own.  The entries only ADD to ABI 5 ----
 *
 * This layer knows nothing about genes or files.
 * Units: a unit is a byte string.  Input: n sample units and m background units, n, m < 2^30, each side given as offsets
 *   (count + 1 of them, uint64) into one text.  The units are taken as given: nothing is deduplicated here.
 * Taking part: a unit takes part when it has 1 .. DCRX_CDR3NET_MAX_LEN (32) bytes, all 'A' .. 'Z'.  A unit of another length is
 *   counted as out of reach, one in reach with another byte as not letters.  n' is the number of sample units that take part, m'
 *   the number of background units that do.
 * Motifs: K is a subset of {2, 3, 4}, given as k_mask (bit k set: k is in K); the trim is (N, C), 0 .. DCRX_CDR3_MOTIF_MAX_TRIM
 *   (16) each.  A unit of L letters has, per k in K, the windows p with N <= p and p + k <= L - C.  A motif is (k, the k letters).
 *   A unit contains a motif when at least one of its windows equals it: a motif that occurs twice in a unit counts once.  A unit
 *   too short for any window still takes part (it counts in n' and m', and it can be drawn).  Motifs are ordered by (k, letters)
 *   ascending; the code of a motif is its letters ('A' = 0 .. 'Z' = 25) as a number to the base 26, the first letter leading, so
 *   that (k, code) ascending is the same order.
 * Counts: cs(motif) = the sample units that take part and contain it; cb(motif) = the background units that take part and
 *   contain it.  The reported motifs are those with cs >= min_count (min_count >= 1), in motif order; `need` is their number.
 * Resampling: R resamples, 0 .. DCRX_CDR3_MOTIF_MAX_RESAMPLES (65535).  Resample r keeps the n' background units that take
 *   part whose key(seed, r, b) are smallest, b the unit's index in the background as given and key the function of "downsample"
 *   above (sample = r, read = b).  The keys of one resample are pairwise distinct: there is no tie rule.  c_r(motif) = the kept
 *   units that contain the motif.  Per reported motif: ge = #{r : c_r >= cs}, sum = the sum over r of c_r, max = the largest
 *   c_r.  n' = m' is legal (every resample is the whole background); n' > m' with R > 0 is DCRX_E_INVALID where the host can
 *   see it.  R = 0 gives cs and cb alone (ge, sum, max 0).
 * Everything is an integer and a function of the input alone: no launch shape, order of arrival or work-space size enters it.
 * Output: rows 0 .. min(need, cap) - 1 of seven caller arrays of `cap` rows — k, code, cs, cb, ge, max (uint32) and sum
 *   (uint64) —, `need` whole whatever `cap` is, and the statistics. */
#define DCRX_CDR3_MOTIF_MAX_TRIM 16
#define DCRX_CDR3_MOTIF_MAX_RESAMPLES 65535
#define DCRX_CDR3_MOTIF_K_ALL 0x1Cu /* k_mask of K = {2, 3, 4} */

typedef struct dcrx_cdr3_motif_stats {
  uint64_t sample_units, sample_take_part, sample_out_of_reach, sample_not_letters;
  uint64_t background_units, background_take_part, background_out_of_reach, background_not_letters;
  uint64_t motifs;        /* distinct motifs with cs >= 1 */
  uint64_t reported;      /* ... with cs >= min_count: `need` */
} dcrx_cdr3_motif_stats_t;

/* Bytes of device work space dcrx_cdr3_motifs_device needs for n sample units, m background units and R resamples; 0 for
 * n or m >= 2^30 and for R above DCRX_CDR3_MOTIF_MAX_RESAMPLES.  The resamples are worked off in chunks: a chunk's kept lists
 * (n indices per resample) and its plane of counts (a row of min(475 228, 90 n) motifs per resample) take 2^25 dwords at most,
 * and a chunk holds 1 .. 64 resamples. */
uint64_t dcrx_cdr3_motifs_work_bytes(uint64_t n, uint64_t m, uint32_t resamples);

/* The primitive, asynchronous on `hip_stream`, everything in device memory: d_s_off n + 1 and d_b_off m + 1 offsets into
 * d_s_text and d_b_text; the seven output arrays of `cap` rows each (they may be NULL where cap is 0); d_need one uint64 and
 * d_stats one dcrx_cdr3_motif_stats_t.  Nothing is copied back and nothing waits.  The steps: a lane per unit packs it as the
 * CDR3 walk packs a string and decides whether it takes part; a lane per unit adds one onto cs (cb) of each of its motifs in a
 * table over all 475 228 motifs (integer atomics whose results are not read); an ordered compaction of the table gives the
 * reported motifs and every motif's row.  Per chunk of resamples: a block per resample finds the resample's threshold — a
 * histogram of the keys' top 8 bits in LDS, then of the next 8 bits among the keys of the threshold's bin while that bin holds
 * more than 512 keys, then the bin's keys written out and the one with the wanted number of smaller keys; keys are computed
 * where they are needed and never stored — and writes the indices of the n' kept units; a lane per kept unit of the chunk
 * adds one per motif of the unit onto the resample's row of the plane; a lane per reported motif folds the chunk's rows into
 * ge, sum and max.  The work is split by kept units: only the n' units of a resample are looked at, not the background's m'.
 * d_work: dcrx_cdr3_motifs_work_bytes(n, m, resamples) bytes, 256-byte aligned; a smaller one is DCRX_E_INVALID, not a launch.
 * DCRX_E_INVALID also for a null argument, a k_mask that is 0 or has a bit outside DCRX_CDR3_MOTIF_K_ALL, a trim above 16,
 * min_count 0 and resamples above 65535; DCRX_E_UNSUPPORTED for n or m >= 2^30.  What only the device can see: with n' > m'
 * and resamples > 0 nothing is resampled (ge, sum and max stay 0; the statistics carry both numbers); offsets that go down
 * are outside the contract. */
int dcrx_cdr3_motifs_device(uint64_t n, const uint64_t *d_s_off, const char *d_s_text, uint64_t m, const uint64_t *d_b_off,
                            const char *d_b_text, uint32_t k_mask, uint32_t ntrim, uint32_t ctrim, uint32_t min_count,
                            uint32_t resamples, uint64_t seed, uint64_t cap, uint32_t *d_k, uint32_t *d_code, uint32_t *d_cs,
                            uint32_t *d_cb, uint32_t *d_ge, uint64_t *d_sum, uint32_t *d_max, uint64_t *d_need,
                            dcrx_cdr3_motif_stats_t *d_stats, void *d_work, uint64_t work_bytes, void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays of the same shapes: checks the arguments (all of the
 * contract's refusals, n' > m' with resamples > 0 among them, and offsets that go down, before any device call), uploads, runs
 * the primitive on the null stream, copies back the rows below min(need, cap), `need` and the statistics. */
int dcrx_cdr3_motifs(uint64_t n, const uint64_t *s_off, const char *s_text, uint64_t m, const uint64_t *b_off, const char *b_text,
                     uint32_t k_mask, uint32_t ntrim, uint32_t ctrim, uint32_t min_count, uint32_t resamples, uint64_t seed,
                     uint64_t cap, uint32_t *k_out, uint32_t *code_out, uint32_t *cs_out, uint32_t *cb_out, uint32_t *ge_out,
                     uint64_t *sum_out, uint32_t *max_out, uint64_t *need_out, dcrx_cdr3_motif_stats_t *stats_out);

/* ---- motif groups (`motifs --groups`): which units hold each of a list of selected motifs, and the specificity groups — the
 * connected components over shared selected motifs and near-identical units (GLIPH's merge of its "local" and "global"
 * halves), on the GPU.  The reference has no counterpart: the contract below is this library's own.  The entries only ADD to
 * ABI 5 ----
 *
 * This layer knows nothing about genes or files.
 * Units: the input of "motifs" above, one side of it: n byte strings given as n + 1 offsets (uint64) into one text, n < 2^30,
 *   taken as given; k_mask and the trim (N, C) as there.  A unit TAKES PART, and CONTAINS a motif, exactly as "motifs" says.
 * Selected motifs: S of them, 0 <= S <= 475 228, given as two arrays (k, code) in strictly ascending motif order (so no motif
 *   twice), every k in K and every code below 26^k.  Anything else is DCRX_E_INVALID where the host entry can see it.
 * Members: row s holds the indices, ascending, of the units that take part and contain selected motif s.  mem_off has S + 1
 *   entries (uint64; mem_off[0] = 0, mem_off[S] = need); mem is filled below `cap` (entries 0 .. min(need, cap) - 1 of the
 *   rows laid end to end), and `need` is reported whole, whatever `cap` is.  n_motifs[i] is the number of selected motifs unit
 *   i holds (0 for a unit that takes no part).
 * Global edges: G is 0, 1 or 2; 0 means none.  Otherwise two units are linked exactly as dcrx_cdr3_neighbours_device links two
 *   nodes under Hamming at distance G when every class is equal: both have 1 .. 32 bytes, one length, and at most G positions
 *   differ (1 .. G between two DISTINCT strings, which is what a table of distinct units holds; two units with the same bytes
 *   are linked as well, as that primitive links them).  Whether a byte is a letter does not matter here: a unit that takes no part for a byte outside 'A' .. 'Z' is linked
 *   all the same.  degree[i] is that primitive's degree (0 with G = 0).  Two choices are made here, and they are choices, not
 *   measured optima: the differing position is NOT restricted to the untrimmed middle of the string (GLIPH restricts it), and V
 *   genes are ignored (this layer has none).
 * Groups: a group is a connected component of the graph on the n units whose edges are the global edges and a link between any
 *   two units that appear in one member row.  Every unit is in exactly one group; a unit with no edge — one out of reach, one
 *   that takes no part and has no global edge, one that holds no selected motif — is a group of its own.  Groups are numbered
 *   0 .. groups - 1 by their smallest unit index, ascending.  Per unit: group_of, n_motifs, degree.  Per group: head (its
 *   smallest unit), units (how many) and weight (the sum of a caller-supplied uint64 weight per unit, modulo 2^64).
 * Everything is an integer and a function of the input alone: no launch shape, order of arrival of an atomic or work-space
 *   size enters a result. */
typedef struct dcrx_cdr3_motif_group_stats {
  uint64_t units, take_part;
  uint64_t selected;          /* S */
  uint64_t member_pairs;      /* (selected motif, unit that holds it) pairs: the members' `need` */
  uint64_t global_edges;      /* unordered pairs of units */
  uint64_t groups, singleton_groups, largest_group;
  uint64_t mixed_groups;      /* groups that hold a global edge AND a member row of two or more units */
  uint64_t rounds;            /* label rounds run, the last one (which moved nothing) included */
} dcrx_cdr3_motif_group_stats_t;

/* Bytes of device work space dcrx_cdr3_motif_members_device needs for n units and `cap` members; 0 for n >= 2^30 and for
 * cap + n >= 2^31.  (The primitive sorts the postings of the rows that begin below `cap`: at most cap + n keys.) */
uint64_t dcrx_cdr3_motif_members_work_bytes(uint64_t n, uint64_t cap);

/* The members primitive, asynchronous on `hip_stream`, everything in device memory: d_off n + 1 offsets into d_text; d_sel_k and
 * d_sel_code S entries each (they may be NULL where S is 0); d_n_motifs n entries; d_mem_off S + 1; d_mem `cap` entries (may be
 * NULL where cap is 0: a counting call, which gives n_motifs, mem_off and need); d_need one uint64.  Nothing is copied back and
 * nothing waits.  The steps: row_of over all 475 228 motifs, scattered from the S selected; a lane per unit packs it and decides
 * whether it takes part ("motifs"' own pack step); a lane per unit counts its selected motifs (n_motifs) and adds one onto
 * its rows' counts (integer atomics whose results are not read); an exclusive sum over the rows: mem_off and need.  With
 * cap > 0: a lane per unit counts its postings in the rows that begin below cap; an exclusive sum over the units; a lane per
 * unit writes (row << 32) | unit keys at its place; a stable radix sort over the keys' 49 significant bits; d_mem is the low
 * halves of the first min(need, cap) keys.  The order never comes from a cursor moved by atomics.
 * d_work: dcrx_cdr3_motif_members_work_bytes(n, cap) bytes, 256-byte aligned; a smaller one is DCRX_E_INVALID, not a launch.
 * DCRX_E_INVALID also for a null argument, a bad k_mask or trim and S above 475 228; DCRX_E_UNSUPPORTED for n >= 2^30 and
 * cap + n >= 2^31.  What only the device can see: a selected (k, code) that is no motif of K is skipped; a motif selected twice
 * and offsets that go down are outside the contract. */
int dcrx_cdr3_motif_members_device(uint64_t n, const uint64_t *d_off, const char *d_text, uint32_t k_mask, uint32_t ntrim,
                                   uint32_t ctrim, uint64_t S, const uint32_t *d_sel_k, const uint32_t *d_sel_code, uint64_t cap,
                                   uint32_t *d_n_motifs, uint64_t *d_mem_off, uint32_t *d_mem, uint64_t *d_need, void *d_work,
                                   uint64_t work_bytes, void *hip_stream);

/* Bytes of device work space dcrx_cdr3_groups_device needs for n units and S member rows; 0 for n >= 2^30 or S above 475 228. */
uint64_t dcrx_cdr3_groups_work_bytes(uint64_t n, uint64_t S);

/* The groups primitive, on `hip_stream`, everything in device memory: the connected components of the n units under a unit-unit
 * adjacency in CSR (d_adj_off n + 1 offsets, d_adj; adj_entries, the number of entries d_adj holds, may be 0 and d_adj then
 * NULL) and S member rows in CSR (d_mem_off S + 1 offsets, d_mem in (row, unit) order; mem_entries, the number of entries d_mem
 * holds, may be 0 and d_mem then NULL; S may be 0 and d_mem_off then NULL).  Any adjacency serves, not the Hamming one alone; an
 * entry of d_mem or d_adj outside 0 .. n - 1 is outside the contract (a member outside is skipped).  Outputs: d_group_of n
 * entries; d_head, d_units, d_weight n entries of room each, filled per group; d_groups one uint32, the number of groups.
 * Rounds of smallest-label propagation until one moves nothing: every row takes the smallest label among its members (a lane per
 * member; consecutive lanes share a row, so the minimum is first taken within the wave, then one atomic per row and wave); every
 * unit takes the smallest among itself, its adjacency and its rows; the labels are followed to their ends.  Then the totals
 * (integer atomics onto the heads) and the heads compacted in unit order.  The atomics' results are not read and the fixed point
 * does not depend on their order.  A round WAITS for the stream once (the word that says whether a label moved); *rounds_out
 * (host, may be NULL) is the number of rounds.  d_work: dcrx_cdr3_groups_work_bytes(n, S) bytes, 256-byte aligned; a smaller
 * one is DCRX_E_INVALID, not a launch.  DCRX_E_INVALID also for a null argument; DCRX_E_UNSUPPORTED for n >= 2^30. */
int dcrx_cdr3_groups_device(uint64_t n, const uint64_t *d_weight, const uint64_t *d_adj_off, const uint32_t *d_adj, uint64_t adj_entries,
                            uint64_t S, const uint64_t *d_mem_off, const uint32_t *d_mem, uint64_t mem_entries, uint32_t *d_group_of,
                            uint32_t *d_head, uint32_t *d_units, uint64_t *d_weight_out, uint32_t *d_groups, uint32_t *rounds_out,
                            void *d_work, uint64_t work_bytes, void *hip_stream);

/* The host entry, synchronous on the current device, on host arrays: checks the arguments (all of the contract's refusals, the
 * order of the selected motifs and offsets that go down among them, before any device call), uploads, runs the members
 * primitive as a counting call, allocates exactly `need` members and runs it again; with distance > 0 the neighbour primitive
 * (every class 0: the degree pass, an adjacency of exactly the entries it takes, the write pass); the groups primitive; copies
 * everything back.  Per unit (n entries each): group_of_out, n_motifs_out, degree_out.  Per group (n entries of room each):
 * head_out, units_out, weight_out.  mem_off_out S + 1 entries; mem_out mem_cap entries (may be NULL where mem_cap is 0), filled
 * only when the members fit (need <= mem_cap); *mem_need_out the need.  The number of groups is stats_out->groups.
 * DCRX_E_INVALID for a null argument, a bad k_mask or trim, a distance above 2, S above 475 228, selected motifs out of order or
 * with a k outside K or a code outside its k, and offsets that go down; DCRX_E_UNSUPPORTED for n >= 2^30 and where the
 * members' need + n reaches 2^31. */
int dcrx_cdr3_motif_groups(uint64_t n, const uint64_t *off, const char *text, const uint64_t *weight, uint32_t k_mask, uint32_t ntrim,
                           uint32_t ctrim, uint64_t S, const uint32_t *sel_k, const uint32_t *sel_code, uint32_t distance,
                           uint32_t *group_of_out, uint32_t *n_motifs_out, uint32_t *degree_out, uint32_t *head_out, uint32_t *units_out,
                           uint64_t *weight_out, uint64_t *mem_off_out, uint32_t *mem_out, uint64_t mem_cap, uint64_t *mem_need_out,
                           dcrx_cdr3_motif_group_stats_t *stats_out);

/* What a handle has settled for its own launches (no counterpart in the reference).  Where the scan kernel takes the tail
 * itself, a handle times the finishing launches of its first calls of a batch-size class (batches of 2^k .. 2^(k+1) - 1 reads,
 * k >= 20) on two settings and keeps the faster for the class: 4096 or 3072 rescue waves for batches below 2^25 reads, 8192 or
 * 4096 from there (`candidates`: the first setting | the second << 16).  rescue_waves = the choice once settled, 0 before (a
 * launch then runs on the first setting or is one of the two samples); launches = the class's calls that took part, counted until
 * the choice settled (calls with cfg flags, and the second pass of orientation `both`, take no part); us_first / us_second =
 * what the samples took (0 before).  The samples are read without waiting, so a caller that queues launches ahead of the device
 * keeps the first setting until they are complete — except, where the caller has allowed it with dcrx_set_tune_wait(tables, 1),
 * for batches of 2^25 reads and more: the fourth call of such a class then waits for the third's finishing launch, once
 * (milliseconds; such batches gain up to 6 % from the choice).  The default is never to wait.
 * orientation: DCRX_ORIENT_REVERSE or DCRX_ORIENT_FORWARD, as in dcrx_cfg_t (the frame whose launches are meant).
 * DCRX_E_INVALID for a null argument.
 * Round 6: where the scan kernel takes the tail, a handle also settles per size class whether list E's entries (one gene to rescue) are
 * finished inside the scan kernel as well (launch_form 4) or by the finishing launch (3): where list E held at most a quarter of the
 * reads of the class's first launch, three launches of each form are timed (events on the dispatches, read without waiting) and
 * the form inside the scan stays if it was at least 1.5 % shorter.  Only calls made once the first launch's lists have been
 * counted and the rescue waves are settled, without events of the caller's (dcrx_set_step_events) and without a tuple sink, count
 * for this: the ninth of them is the first timed one. */
typedef struct dcrx_tune_state {
  uint32_t rescue_waves, launches;
  float us_first, us_second;
  uint32_t launch_form;      /* the frame's last call, whatever its size: 0 none yet, 1 the three-launch form (tag sets or shapes the
                                v2 kernels do not serve), 2 the v2 kernels with the tail a role of the finishing launch, 3 the v2
                                kernels with the tail inside the scan kernel, 4 the same with list E's entries finished inside the scan kernel as
                                well (chosen per size class from the share of list-E entries in the class's first launch) */
  uint32_t candidates;
} dcrx_tune_state_t;
int dcrx_tune_state(const dcrx_tables_t *tables, int orientation, uint64_t n_reads, dcrx_tune_state_t *out);
/* allow != 0: dcrx_decombine_device may wait once per big-batch size class as described above (0, the default: never). */
int dcrx_set_tune_wait(dcrx_tables_t *tables, int allow);

/* The persistent kernels of dcrx_decombine_device normally fill every compute unit; n_cus of
 * them are left free from the next call on (for a collective running on another stream). */
int dcrx_set_reserved_cus(dcrx_tables_t *tables, uint32_t n_cus);

/* ---- multi-GPU: RCCL over xGMI, bound directly (SURVEY.md 8(b) dcrx_decombine_sharded, 8(e)) -----------------------
 * The reference has no counterpart (one process, one Counter: decombine.py:598, README.md:370-376 "submit many jobs").
 * Reads are sharded over the ranks in contiguous ranges (rank r of W owns reads [r N / W, (r + 1) N / W): concatenating the
 * ranks' outputs in rank order is the reference's input order, outdata.append :1039), every rank runs the hot path on its own
 * GPU, and ONE exchange follows: the ranks' counts of decombined reads (all-gather), their tuple messages — the
 * dcrx_set_tuple_sink message: a bitmap of the shard's reads and the narrow tuples of the decombined ones — to rank 0 in
 * exact sizes (grouped send / receive), the uint64[DCRX_N_COUNTERS] summed over the ranks (all-reduce).
 * librccl is opened on the first call of this section (by soname: a process that already holds an RCCL shares it); a caller
 * that never comes here never loads it.  DCRX_E_UNSUPPORTED when it cannot be opened.
 *
 * A communicator: one process per GPU — rank 0 draws an id (dcrx_comm_unique_id), carries its DCRX_COMM_ID_BYTES bytes to the
 * other ranks by whatever means it has (a file, a socket, an environment variable of the launcher), and every rank calls
 * dcrx_comm_create on its own device (dcrx_set_device first) — or one process for all GPUs: dcrx_comm_create_all fills
 * out[0 .. world) (ncclCommInitAll; devices == NULL: 0 .. world - 1). */
#define DCRX_COMM_ID_BYTES 128
enum dcrx_comm_op { DCRX_COMM_SUM = 0, DCRX_COMM_MAX = 1 };
typedef struct dcrx_comm dcrx_comm_t;
int dcrx_comm_available(void);                        /* 1 when librccl could be opened */
int dcrx_comm_unique_id(uint8_t *id /* DCRX_COMM_ID_BYTES */);
int dcrx_comm_create(const uint8_t *id, int world, int rank, dcrx_comm_t **out);
int dcrx_comm_create_all(int world, const int *devices, dcrx_comm_t **out /* [world] */);
void dcrx_comm_destroy(dcrx_comm_t *comm);
int dcrx_comm_info(const dcrx_comm_t *comm, int *world, int *rank, int *device);
/* The pieces, asynchronous on `hip_stream`, device memory throughout — for a caller that pipelines steps (bench.py:
 * the transfers of step k beside the scan of step k + 1).  gather_v: every rank but `root` sends send_bytes from d_send;
 * the root receives recv_bytes[r] into d_recv[r] from every r != root, all in one group (its own message stays where it
 * is; d_recv and recv_bytes are read on the root only). */
int dcrx_comm_allreduce_u64(dcrx_comm_t *comm, const uint64_t *d_in, uint64_t *d_out, uint64_t n, int op, void *hip_stream);
int dcrx_comm_allreduce_f64(dcrx_comm_t *comm, const double *d_in, double *d_out, uint64_t n, int op, void *hip_stream);
int dcrx_comm_allgather(dcrx_comm_t *comm, const void *d_in, void *d_out /* world x bytes_per_rank */, uint64_t bytes_per_rank, void *hip_stream);
int dcrx_comm_gather_v(dcrx_comm_t *comm, const void *d_send, uint64_t send_bytes, void *const *d_recv, const uint64_t *recv_bytes,
                       int root, void *hip_stream);
int dcrx_comm_barrier(dcrx_comm_t *comm, void *hip_stream);      /* an all-reduce of one word, then the stream is waited for */
/* Host memory in and out, synchronous (staged through device memory): sizes, error flags, a Counter's keys. */
int dcrx_comm_allgather_host(dcrx_comm_t *comm, const void *h_in, void *h_out /* world x bytes_per_rank */, uint64_t bytes_per_rank);
int dcrx_comm_allreduce_host_u64(dcrx_comm_t *comm, uint64_t *h_inout, uint64_t n, int op);
/* One step of a sharded run in one call, on every rank: dcrx_decombine_device on this rank's shard (device memory, as
 * there) with the tuple sink on d_message (room for dcrx_tuple_message_bytes(layout, n_slots, n_slots); n_slots >= the
 * shard's reads); then the exchange above.  On return the stream holds — not yet waited for — the transfers and the
 * all-reduce: d_counters will be the JOB's counters on every rank, and on rank 0 d_gathered[r] rank r's message for r > 0
 * (d_gathered[0] is not touched: rank 0's own message is d_message; d_gathered is read on rank 0 only).  n_hits_by_rank
 * (host, [world]) is filled before the call returns: the one wait inside (the counts decide the transfers' sizes).
 * Unpacking a message: bitmap of n_slots bits, then the tuples in read order (dcrx_tuple_layout_t above). */
int dcrx_decombine_sharded(dcrx_tables_t *tables, dcrx_comm_t *comm, const dcrx_cfg_t *cfg, const dcrx_batch_t *device_shard,
                           dcrx_record_t *d_records, uint64_t *d_counters, const dcrx_tuple_layout_t *layout, void *d_message,
                           uint64_t n_slots, void *const *d_gathered, uint64_t *n_hits_by_rank, void *hip_stream);

/* ---- device plumbing for callers without a HIP binding of their own ---- */
int dcrx_device_count(void);
int dcrx_set_device(int device);
int dcrx_device_name(char *buf, size_t cap);
int dcrx_malloc_device(void **ptr, size_t bytes);
int dcrx_free_device(void *ptr);
/* Page-locked host memory: dcrx_decombine copies straight from a `packed` buffer and into a `records` buffer that live in
 * such memory (its own or any other the HIP runtime has pinned), without the staging copies pageable buffers need. */
int dcrx_malloc_host(void **ptr, size_t bytes);
int dcrx_free_host(void *ptr);
int dcrx_memcpy_h2d(void *dst_device, const void *src_host, size_t bytes);
int dcrx_memcpy_d2h(void *dst_host, const void *src_device, size_t bytes);
int dcrx_memset_device(void *dst_device, int value, size_t bytes);
int dcrx_synchronize(void);
/* HIP events on a stream, for timing the launches above where they run */
int dcrx_event_create(void **event);
int dcrx_event_destroy(void *event);
int dcrx_event_record(void *event, void *hip_stream);
int dcrx_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
int dcrx_event_synchronize(void *event);
int dcrx_event_create_ordering(void **event);      /* an event without timestamps (hipEventDisableTiming): for ordering streams, cheaper to record */
/* streams of the caller's own, and copies on them (a sharded caller's side stream for the exchange) */
int dcrx_stream_create(void **hip_stream);
int dcrx_stream_destroy(void *hip_stream);
int dcrx_stream_synchronize(void *hip_stream);
int dcrx_stream_wait_event(void *hip_stream, void *event);
int dcrx_memcpy_d2h_async(void *dst_host, const void *src_device, size_t bytes, void *hip_stream);
int dcrx_memcpy_d2d_async(void *dst_device, const void *src_device, size_t bytes, void *hip_stream);
int dcrx_memset_device_async(void *dst_device, int value, size_t bytes, void *hip_stream);

int dcrx_abi_version(void);
const char *dcrx_last_error(void);
/* 1 when the HIP kernels are compiled in (always, in this library), and the
 * gfx target they were built for */
const char *dcrx_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* DCRX_H */
