/* mahip.h -- thin C ABI between the host C code and the hand-written HIP kernels (gfx950).
 *
 * One mahip_ctx_t per GPU (one process per GPU).  Hits live in HBM as SoA columns between calls; every
 * pass is an in-place "flag + rewrite" pass (no compaction until something is exported), arcs are a dense
 * SoA edge list + CSR index.  Each entry cites the reference function whose result it reproduces
 * (file:line under the reference tree).  All functions return 0 on success, non-zero on failure with the
 * message available from mahip_strerror(); there is NO CPU fallback: without a usable GPU mahip_create fails.
 */
#ifndef MAHIP_H
#define MAHIP_H

#include <stddef.h>
#include <stdint.h>
#include "miniasm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mahip_ctx mahip_ctx_t;

int mahip_device_count(void);
/* stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL to create a private one */
mahip_ctx_t *mahip_create(int device, void *stream);
void mahip_destroy(mahip_ctx_t *c);
const char *mahip_strerror(void);
int mahip_sync(mahip_ctx_t *c);
/* one trivial kernel launch + wait (start-up timing: the first launch of a process loads the code object) */
int mahip_first_launch(mahip_ctx_t *c);

/* ---- hits ------------------------------------------------------------------------------------------ */
/* n unsorted (or sorted) 32-byte ma_hit_t records, reads numbered [0,n_seq).  upload = H2D copy of a host
 * array; adopt = the records already sit in HBM at d_hits (not owned, never written). */
int mahip_hits_upload(mahip_ctx_t *c, const ma_hit_t *h, size_t n, uint32_t n_seq);
int mahip_hits_adopt(mahip_ctx_t *c, const void *d_hits, size_t n, uint32_t n_seq);
/* Multi-GPU: this context owns the hits whose query id lies in [q_beg,q_end); call before sort/index. */
int mahip_set_shard(mahip_ctx_t *c, uint32_t q_beg, uint32_t q_end);
/* Read ranges that hold equally many hits: bounds[0..world], rank r owns [bounds[r], bounds[r+1]).  mahip_hits_balance computes the table from the unsorted
 * records in the context (identical on every rank that holds the whole input) and keeps it; mahip_set_shard_bounds installs a table made elsewhere;
 * the orchestrator (host/sharded.c) uses the table of its world size when there is one, equal read counts otherwise.  A table describes ONE upload, like the
 * hints and the positions: every mahip_hits_upload / mahip_hits_adopt forgets it -- install it (again) after the records. */
int mahip_hits_balance(mahip_ctx_t *c, int world, uint32_t *bounds);
int mahip_set_shard_bounds(mahip_ctx_t *c, const uint32_t *bounds, int world);
const uint32_t *mahip_shard_bounds(mahip_ctx_t *c, int *world);

/* ---- PAF text ingest on the device (replaces paf.c:34-67 paf_parse/paf_read + sdict.c:27-45 sd_put + hit.c:70-101, the part of
 * ma_hit_read before the sort).  Load the whole (decompressed) text, parse: afterwards the context holds the unsorted hit
 * records exactly as the reference has them before ma_hit_sort (as after mahip_hits_upload) and the read-name dictionary
 * with the reference's ids (dense, in order of first appearance, first length wins). */
typedef struct {
	uint64_t n_lines;         /* text lines */
	uint64_t n_records;       /* lines with >= 10 columns = what the reference logs as "read %ld hits" (hit.c:102) */
	uint64_t n_stored_lines;  /* lines passing the span/match filter (hit.c:85) */
	uint64_t n_hits;          /* records stored (mirrored hits included) */
	uint64_t name_bytes;      /* bytes mahip_paf_names() writes (names NUL-terminated, back to back, in id order) */
	uint32_t n_seq, max_qs;   /* reads in the dictionary; upper bound of the stored query starts */
	uint32_t n_excl;          /* -R: reads excluded as clearly contained (what the reference logs as "dropped %d contained reads", hit.c:66) */
} mahip_paf_info_t;
int mahip_paf_load_mem(mahip_ctx_t *c, const void *text, size_t nbytes);   /* text in host memory */
int mahip_paf_load_fd(mahip_ctx_t *c, int fd, size_t nbytes);              /* bytes [0,nbytes) of an open plain file, read straight into pinned staging */
int mahip_paf_parse(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, mahip_paf_info_t *info);
/* the same with the -R pre-filter folded in (hit.c:38-68 ma_hit_no_cont + the exclusion test of hit.c:86): names of reads that some line shows
 * to be clearly contained are excluded before ids are given out; lines touching them are dropped */
int mahip_paf_parse_excl(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, int no_cont, int max_hang, float int_frac, mahip_paf_info_t *info);
/* Sharded ingest ("ingest routing option B"; host/ingest_sharded.c): every rank loads and parses ITS byte range of the text (ranges in rank order,
 * cut at line starts) and the ranks exchange what the reference's sequential reader carries across a range border: line counts (occurrence numbers count lines
 * of the whole file), the `bl` a 10-column line inherits (paf.c:54), and the distinct names of every range with their first appearances, merged into ONE
 * dictionary with the reference's ids on every rank (sdict.c:27-45).  A bgzip-compressed file: mahip_bgzf_load_fd_range (below) in the place of
 * mahip_paf_load_fd_range; plain gzip, stdin and -R are ingested whole on every rank, and every rank walks a bgzip file's whole member chain.  Afterwards the context holds the records of its own lines (global ids); info: line /
 * record counts are totals over the ranks, n_hits is this rank's.  Collective: needs a communicator (mahip_comm_init*); -R is not served in this mode. */
int mahip_paf_load_fd_range(mahip_ctx_t *c, int fd, size_t off, size_t nbytes);
int mahip_paf_parse_sharded(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, mahip_paf_info_t *info);
/* after mahip_paf_parse_sharded: every record to the rank that owns its query read (read ranges with equally many hits, from the ranks' summed per-read
 * counts: kept as the context's shard bounds), with its position in the record sequence of the whole input.  The context then holds its own records in input
 * order, as ma_pipeline_head_sharded(full_input = 0) wants them.  *n_total = records of all ranks; *bytes_sent = what this rank sent away. */
int mahip_hits_route(mahip_ctx_t *c, uint64_t *n_total, uint64_t *bytes_sent);
int mahip_paf_names(mahip_ctx_t *c, char *names, uint32_t *lens);
/* the same as ready-made sd_seq_t records (sdict.h:6-10) whose name pointers point into `names` (a host block of name_bytes): seqs16[n_seq * 16 bytes] */
int mahip_paf_seqs(mahip_ctx_t *c, char *names, void *seqs16, uint64_t *tot_len);          /* names[name_bytes], lens[n_seq] = first-seen read lengths */
int mahip_paf_release(mahip_ctx_t *c);                                      /* free the text and the per-line columns */
/* For stage tests: what the LAST mahip_paf_parse* of this context decided and counted (host bookkeeping, read-only), and its per-line columns.  Both are valid
 * from the parse until mahip_paf_release and fail afterwards.  n_gran: KiB granules of the text (the appended newline of an open last line included);
 * tile_k / n_tiles: granules per tile, tiles; tile_form: KiB of text a block of the tile parser stages / 16 (1 or 2); n_odd: lines the tile parser left to the
 * byte-wise routine, odd_ran: that kernel was launched; n_long: stored lines with a name that is not 1..8 bytes; dict_form: the short-key or the text-comparing
 * name table (0: no stored line, no table); the insert pass ran n_attempts times, attempt a on a table of cap[a] slots, and ended as end[a] says (LOAD: more
 * than cap / 2 distinct names; PROBES: a probe sequence ran out); n_distinct: names the last attempt counted (with -R: before the exclusion); bl_pass: the
 * pass that hands 10-column lines their stale `bl` ran; n_excl as in mahip_paf_info_t.  After mahip_paf_parse_sharded: this rank's range, bl_pass 0. */
enum { MAHIP_PAF_DICT_NONE = 0, MAHIP_PAF_DICT_SHORT = 1, MAHIP_PAF_DICT_TEXT = 2 };
enum { MAHIP_PAF_TAB_OK = 0, MAHIP_PAF_TAB_LOAD = 1, MAHIP_PAF_TAB_PROBES = 2 };
typedef struct {
	uint64_t n_lines, n_odd, n_long, n_distinct;
	uint32_t n_gran, tile_k, n_tiles, n_excl;
	int tile_form, open_line, odd_ran, dict_form, bl_pass, n_attempts;
	uint32_t cap[4];
	int end[4];
} mahip_paf_report_t;
int mahip_paf_last(mahip_ctx_t *c, mahip_paf_report_t *out);
/* host arrays, any of them NULL: flags[n_lines] (bit0 valid, bit1 stored, bit2 has column 11, bit3 rev, 0x10: the query name is that of the stored line in
 * front of it and the tile parser saw it), odd[n_lines] (1: the line went through the byte-wise routine; needs mahip_paf_keep_odd), nums[8][n_lines] (ql qs qe tl
 * ts te ml bl), tnoff / qlen / tlen[n_lines] (target-name offset in the line, name lengths), lstart[n_lines + 1], tfirst[n_tiles] (start of the first line
 * that ends in each tile).  Columns of lines with fewer than 10 columns are unspecified. */
int mahip_paf_cols_download(mahip_ctx_t *c, uint8_t *flags, uint8_t *odd, uint32_t *nums, uint32_t *tnoff, uint32_t *qlen, uint32_t *tlen, uint64_t *lstart, uint64_t *tfirst);
/* on: every following parse of this context copies, between the tile parser and the byte-wise kernel, which lines wait for the latter (one D2H copy of the
 * flags: for tests, not for production runs).  Off by default. */
int mahip_paf_keep_odd(mahip_ctx_t *c, int on);
uint32_t mahip_paf_max_qs(mahip_ctx_t *c);                                  /* info.max_qs of the last parse (a sort hint for later mahip_hits_adopt calls) */
/* ---- the same ingest, piece by piece (what the reference's reader does by streaming: paf.c:9-20 paf_open over kseq.h:59-157, one line at a time through a
 * 16-KiB buffer).  The pieces of one text arrive in order; the context never holds more text than one piece.  begin ... piece* ... end leaves the context as
 * mahip_paf_parse leaves it on the concatenated text: the same records in the same order (hit.c:70-101), the same ids and first-seen lengths (sdict.c:27-45
 * sd_put), the same mahip_paf_info_t; mahip_paf_names, mahip_paf_seqs, mahip_paf_release, mahip_hits_sort and what follows work as after a whole parse (records
 * are a line's record and its mirror side by side: the run stride is set to 2, or to 1 without bi_dir).  mahip_paf_last and mahip_paf_cols_download describe the
 * LAST PIECE THAT HAD TEXT (zeros when none had).  -R is served by mahip_paf_stream_begin_excl (below: provisional ids, renumbered at the end).  Not served:
 * contexts with a communicator.
 * mahip_paf_stream_begin (hit.c:76-79: the dictionary and the record array start empty): a stream the context still holds is dropped.
 * mahip_paf_stream_piece_mem (hit.c:80-100 on the lines of the piece): a piece is WHOLE LINES -- one that is not the last, has bytes and does not end with '\n'
 * is an error; the last piece (last != 0) may end without a newline and gets the virtual one a whole parse gives its text (kseq.h:139-144: the rest of the
 * stream is a line); pieces of 0 bytes are legal anywhere; nothing may follow the last piece.  MA_PAF_MAX_BYTES counts the piece's own bytes.  A 10-column
 * line takes the `bl` of the last 11-column line of this or ANY earlier piece (paf.c:54 leaves the field alone).  After an error: mahip_paf_stream_abort.
 * mahip_paf_stream_end (hit.c:101-102): adopts the records and hands over the dictionary; legal without any piece (everything zero).
 * mahip_paf_stream_abort: everything the stream holds goes back to the pool (legal without a stream).
 * MA_STREAM_DICT_CAP_LOG2 / MA_STREAM_REC_CAP: the first capacity of the name table (slots, log2) and of the record buffer (records); both grow (tests). */
typedef struct {
	uint64_t n_pieces, n_empty;       /* pieces seen; of them, pieces of 0 bytes */
	uint64_t n_short, n_text;         /* pieces whose local name table took MAHIP_PAF_DICT_SHORT / MAHIP_PAF_DICT_TEXT */
	uint64_t n_inherited;             /* pieces whose FIRST line is a 10-column line that took its bl from an earlier piece */
	uint32_t tab_cap, n_rebuilds;     /* slots of the persistent name table now; times it was rebuilt larger from the names so far */
	uint32_t n_fold_repeats;          /* folds repeated on a rebuilt table because a probe sequence had run out */
	uint32_t n_rec_grow;              /* times the record buffer was replaced by a larger one */
	uint32_t last_local, last_new;    /* the last piece with text: its distinct names; of them, names no earlier piece had */
	uint32_t last_before;             /* ... the bl its 10-column lines in front of its first 11-column line inherit */
	int last_form;                    /* ... its MAHIP_PAF_DICT_* */
	double t_upload, t_parse, t_fold; /* seconds so far: text to the device; the stages of the parse; the fold into the persistent dictionary */
	uint32_t n_arena_grow, n_ids_grow; /* pieces for which the names arena / any of the three per-id arrays was replaced by a larger one (the first buffers replace none) */
} mahip_paf_stream_report_t;
int mahip_paf_stream_begin(mahip_ctx_t *c, int min_span, int min_match, int bi_dir);
int mahip_paf_stream_piece_mem(mahip_ctx_t *c, const void *text, size_t nbytes, int last);
int mahip_paf_stream_end(mahip_ctx_t *c, mahip_paf_info_t *info);
int mahip_paf_stream_abort(mahip_ctx_t *c);
int mahip_paf_stream_last(mahip_ctx_t *c, mahip_paf_stream_report_t *out);   /* valid from begin until the next begin, abort or mahip_paf_release */
/* -R in the stream (hit.c:38-68 + hit.c:86): begin_excl with no_cont != 0 ... end leaves the context as mahip_paf_parse_excl leaves it on the
 * concatenated text, n_excl included.  One pass: names get PROVISIONAL ids while pieces arrive; every stored line gives its verdict against them (a flag per
 * id, 0 -> 1 only); a stored line that touches an id flagged so far is dropped at once; mahip_paf_stream_end retires the records a later flag killed, renumbers
 * the surviving names by first appearance among the surviving lines and rebuilds the dictionary in that order (a name's first-seen length is the one of its
 * first SURVIVING line).  Until then the stream holds the records of lines that die late, and 8 bytes a record for the lengths: peak_records against
 * info.n_hits is what the single pass costs.  no_cont == 0: mahip_paf_stream_begin, to the byte.  MA_STREAM_NOCONT_EARLY=0: no early drop (tests; same result). */
typedef struct {
	uint64_t n_early_lines;           /* stored lines dropped in their own piece: they touched a name flagged by then */
	uint64_t n_late_records, n_late_lines; /* records retired at the end, and the lines they were */
	uint64_t peak_records;            /* the most records the stream ever held */
	uint32_t n_flagged;               /* names flagged (= info.n_excl) */
	uint32_t n_renumbered;            /* names that got an id at the end (= info.n_seq) */
	uint32_t n_flag_grow, n_lens_grow; /* times the flag array / the lengths column was replaced by a larger one (the first buffers replace none) */
} mahip_paf_stream_excl_report_t;
int mahip_paf_stream_begin_excl(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, int no_cont, int max_hang, float int_frac);
int mahip_paf_stream_excl_last(mahip_ctx_t *c, mahip_paf_stream_excl_report_t *out); /* valid as mahip_paf_stream_last; all zero without no_cont (but peak_records) */
/* read-only, between begin and end: the persistent name table as it stands, report.tab_cap words of tag(32) | id, all ones = free (no slots before the first
 * piece that stored a line).  Between pieces no word holds a provisional claim (bit 31 of the low word).  For tests. */
int mahip_paf_stream_tab_download(mahip_ctx_t *c, uint64_t *slots);
int mahip_hits_raw_download(mahip_ctx_t *c, ma_hit_t *out);                 /* the unsorted records held by the context (n_hits of them) */
/* device-to-device: the unsorted records whose query id lies in [q_beg,q_end), in input order, into d_dst (NULL: only count
 * them); *n_out = their number.  Lets a caller keep the records of one read-range shard (bench.py, multi-GPU set-up). */
int mahip_hits_raw_extract(mahip_ctx_t *c, uint32_t q_beg, uint32_t q_end, void *d_dst, size_t *n_out);
/* the same, and (d_pos != NULL, device) the position each extracted record had in this context's input */
int mahip_hits_raw_extract_pos(mahip_ctx_t *c, uint32_t q_beg, uint32_t q_end, void *d_dst, uint32_t *d_pos, size_t *n_out);
/* A context that holds only the records of its read range (mahip_set_full_input(c, 0)) can take part in the repair of the reference's HIT order
 * (hit.c:19-22: an unstable in-place sort -- the order of tied records is a function of the order of ALL records) only if it knows where its records
 * stood in the whole input: pos[i] < n_total (the records of all ranks), distinct over the ranks, increasing on a rank.  The ranks then put the keys of
 * the whole input together (two all-gathers, only when the tie census asks for it) and every rank runs the walk.  Copied (host or device array); like
 * the hints it describes one upload/adopt.  Without positions such a context leaves tied hits in the stable order and reports `unrepaired`. */
int mahip_hits_set_positions(mahip_ctx_t *c, const uint32_t *pos, int on_device, uint64_t n_total);
int mahip_hits_have_positions(mahip_ctx_t *c);
/* for stage tests: the positions the context holds (one word per record it was handed: as many as mahip_hits_raw_download writes right after the upload /
 * adopt / route) into out (host, may be NULL), *n_total = what mahip_hits_set_positions or mahip_hits_route said the ranks hold together.  Read-only; fails
 * when no positions are set. */
int mahip_hits_positions_download(mahip_ctx_t *c, uint32_t *out, uint64_t *n_total);

/* optional: an upper bound of the query starts (e.g. the longest read) lets the on-demand (qid,qs) sorts (hit dumps, push order
 * of the arcs) plan their digits without a sweep over the records; 0 = unknown */
int mahip_set_hints(mahip_ctx_t *c, uint32_t max_qs);
/* optional: how the records of one query's own PAF lines stand in the array: 2 = record and mirror side by side (what ma_hit_read stores with bi_dir, hit.c:87-98),
 * 1 = no mirrored records, 0 = unknown (default).  With 1 or 2 mahip_hits_sort sorts RUNS of records (about half as many keys at stride 2) and expands them
 * afterwards; the result is the same grouping in input order, and it falls back to sorting records by itself when the hint does not fit the data.  Describes one
 * upload/adopt, like the other hints. */
int mahip_set_run_stride(mahip_ctx_t *c, int stride);
uint64_t mahip_hits_sorted_runs(mahip_ctx_t *c); /* elements of the last mahip_hits_sort if it sorted runs, else 0 */
/* What the LAST mahip_hits_sort of this context did (host bookkeeping, read-only; the tests assert from it that a case reached the path and the digit plan it
 * was built for).  path: what the sort's elements were and who counted the first digit (0: no sort yet, or no record to sort).  fallback: a run stride was set
 * and the records were sorted all the same -- NOT_TRIED: a shard, or no dictionary size (n_seq = 0); FIELD_WIDTH: id, position and length do not fit one word;
 * ID_RANGE: an id >= n_seq in the input; FEW_RUNS: more than three runs per four records; INTERLEAVED: two runs of one read overlap (k_runs_expand).
 * n_elem: sorted elements (runs, or this context's records); n_runs_seen: runs k_hit_keys_runs counted (0: not run).  n_pass radix passes over the id bits,
 * pass p on `bits[p]` bits from bit `shift[p]`; fixed7 bit p: the pass ran the scatter with its 7-bit width at compile time; groups: the last pass wrote the
 * group starts (else k_runs_expand or k_hit_goff made them). */
enum { MAHIP_SORT_NONE = 0, MAHIP_SORT_RUNS = 1, MAHIP_SORT_RECORDS_FUSED_HIST = 2, MAHIP_SORT_RECORDS_PLAIN = 3 };
enum { MAHIP_RUNS_NO_FALLBACK = 0, MAHIP_RUNS_NOT_TRIED = 1, MAHIP_RUNS_FEW_RUNS = 2, MAHIP_RUNS_ID_RANGE = 3, MAHIP_RUNS_INTERLEAVED = 4, MAHIP_RUNS_FIELD_WIDTH = 5 };
typedef struct { int path, fallback; uint64_t n_elem, n_runs_seen; int n_pass, bits[8], shift[8]; uint32_t fixed7; int groups; } mahip_sort_info_t;
int mahip_sort_last(mahip_ctx_t *c, mahip_sort_info_t *out);
/* for stage tests: the resident layout the sort leaves (the pending gather is run first): sidx[n_hits] = input position of the record in every slot,
 * goff[n_seq + 1] = first slot of every read's group.  Only after mahip_hits_sort. */
int mahip_hits_layout_download(mahip_ctx_t *c, uint32_t *sidx, uint32_t *goff);
/* Bulk copies between pageable host memory and device memory at PCIe speed: worker threads stage slices through
 * pinned slots while their DMAs run (a plain hipMemcpy of pageable memory is staged by one runtime thread).
 * Synchronous; ordered after the work already queued on the context's stream.  MA_XFER_THREADS sets the workers. */
int mahip_memcpy_h2d(mahip_ctx_t *c, void *d_dst, const void *h_src, size_t bytes);
int mahip_memcpy_d2h(mahip_ctx_t *c, void *h_dst, const void *d_src, size_t bytes);
/* for stage tests: bytes [off, off + nbytes) of an open file -> device memory at d_dst, the road the PAF / reads-file loaders take (pread into the workers'
 * pinned slots; staged at every size).  -1 when the file ends early; what d_dst holds then is undefined, nothing of the copy is still in flight. */
int mahip_memcpy_fd2d(mahip_ctx_t *c, void *d_dst, int fd, size_t off, size_t nbytes);
/* for stage tests: what the LAST bulk copy of this context did (host bookkeeping, read-only; any copy the library made through the staged-copy code counts,
 * its own uploads and downloads included).  road: the runtime's own hipMemcpyAsync (memory to memory below 8 MiB), or staged through the workers' pinned 4 MiB
 * slots from memory / from a file.  slices: 4 MiB slices (0 on the runtime road); workers: threads that dealt them (0 on the runtime road).  A copy of 0 bytes
 * does nothing and is not recorded. */
enum { MAHIP_XFER_NONE = 0, MAHIP_XFER_RUNTIME = 1, MAHIP_XFER_STAGED_MEM = 2, MAHIP_XFER_STAGED_FILE = 3 };
typedef struct { int road, to_device; uint64_t bytes, slices; int workers; } mahip_xfer_info_t;
int mahip_xfer_last(mahip_ctx_t *c, mahip_xfer_info_t *out);
/* Tie order.  The reference's two sorts (ksort.h:134-183, used at hit.c:21 and asg.c:24) are an in-place MSD radix sort that
 * leaves records with equal keys in an order that is a sequential function of the whole input; the device sorts are stable.
 * The difference is only observable through arcs with equal (u,len) keys, so:
 *   mode 2 (default, "auto"): after the arc sort a census counts (u,len) tie groups.  None: the stable order is provably the
 *           reference's result (whatever the order of tied hits was).  Some: the reference's order is reproduced -- a host walk
 *           over the arc keys (squeezed ids, as the reference sorts them) and, only when two arcs were pushed from hits with
 *           equal (qid,qs), over the hit keys too; the device re-gathers.  Hit dumps (mahip_hits_download) are put in the
 *           reference's order when tied hits exist.
 *   mode 1: the same repair, unconditionally.      mode 0: never (stable total order (key, input position)).
 * Initial value: MA_EXACT_TIES in the environment (unset = 2).  On a shard (mahip_set_shard) the census and the repair run after the
 * arc exchange, driven by the orchestrator (host/sharded.c; the split entry points are listed with the sharded building blocks). */
int mahip_set_exact_ties(mahip_ctx_t *c, int mode);
typedef struct {
	uint64_t arc_tie_groups;   /* groups of >= 2 arcs with equal (u,len) after the last ma_sg_gen */
	uint64_t arc_tie_arcs;     /* arcs in such groups */
	uint64_t push_conflicts;   /* consecutive pushed arcs whose hits had equal (qid,qs): the hit order matters */
	uint64_t hit_ties;         /* hits with the same (qid,qs) as their predecessor (only counted when needed, else 0) */
	int arc_walk, hit_walk;    /* 1 if the reference's arc / hit order was computed on the host for the last graph */
	int unrepaired;            /* 1 if tie groups exist and the stable order was kept (mode 0, or a shard) */
	uint64_t push_conflicts_seen; /* of push_conflicts: those the reference's arc sort can turn into a difference (the two arcs part in a bucket of its radix passes that
	                                 * is walked and holds a tie group, or in an insertion-sorted one where one of them has a twin, csrc/graph.hip); 0 of them => the hit
	                                 * walk is not needed and not done */
	uint64_t hit_walk_reads;      /* hit_walk: reads inside whose hit groups the walk's order was taken (the reads with a conflict in sight; every other read keeps the
	                                 * stable order); 0 = the whole order was taken */
} mahip_tie_info_t;
int mahip_tie_stats(mahip_ctx_t *c, mahip_tie_info_t *out);
/* hit.c:19-22 ma_hit_sort.  The resident layout is GROUPED by query id (stable LSD radix sort on the id bits -> SoA + group offsets),
 * input order inside a group: ma_hit_sub / cut / flt / contained do not look at the order inside a group (hit.c:109-160 sorts its own
 * events).  The (qid, qs) order of ma_hit_sort -- with the reference's order of equal keys, see "Tie order" above -- is produced where
 * it can be observed: mahip_hits_download sorts the slots' original keys on demand, mahip_sg_finish orders the pushed arcs. */
int mahip_hits_sort(mahip_ctx_t *c);
/* same layout change without sorting (input already grouped by query id: the per-symbol ABI path) */
int mahip_hits_index(mahip_ctx_t *c);

/* hit.c:109-160 ma_hit_sub into sub slot 0 or 1 */
int mahip_hits_sub(mahip_ctx_t *c, int min_dp, float min_iden, int end_clip, int slot, size_t *n_remained);
/* hit.c:162-193 ma_hit_cut against sub slot */
int mahip_hits_cut(mahip_ctx_t *c, int slot, int min_span, size_t *n_live);
/* hit.c:195-216 ma_hit_flt (int_frac fixed at .5 there) */
int mahip_hits_flt(mahip_ctx_t *c, int slot, int max_hang, int min_ovlp, size_t *n_live, float *cov);
/* hit.c:218-223 ma_sub_merge: slot0 <- compose(slot0, slot1) */
int mahip_sub_merge(mahip_ctx_t *c);
/* hit.c:225-256 ma_hit_contained (+ hit.c:24-36 mark_unused, sdict.c:69-86 squeeze map).
 * seq_del: optional host array [n_seq] of reads already flagged d->seq[i].del. */
int mahip_hits_contained(mahip_ctx_t *c, const ma_opt_t *opt, const uint8_t *seq_del, uint32_t *n_seq_new, size_t *n_live);

/* Fused forms used by the resident pipeline (same results, fewer sweeps over the hits):
 *   cutflt_sub    : hit.c:162-216 (ma_hit_cut against cut_slot, then ma_hit_flt) applied inside the coverage pass that
 *                   computes out_slot (hit.c:109-160) -- the hits are already in registers there;
 *   cut_contained : the second ma_hit_cut (against cut_slot) + the flag pass and the squeeze MAP of ma_hit_contained
 *                   (against slot 0); the squeeze of the hit array itself is postponed to ma_sg_gen / hits_download. */
int mahip_hits_cutflt_sub(mahip_ctx_t *c, int cut_slot, int min_span, int max_hang, int min_ovlp, int min_dp, float min_iden, int end_clip,
                          int out_slot, size_t *n_cut, size_t *n_flt, float *cov, size_t *n_remained);
int mahip_hits_cut_contained(mahip_ctx_t *c, int cut_slot, int min_span, const ma_opt_t *opt, size_t *n_cut, uint32_t *n_seq_new);
/* its two halves for the sharded mode: the r_cont / r_used flags are max-all-reduced across ranks in between */
int mahip_hits_cut_contained_flags(mahip_ctx_t *c, int cut_slot, int min_span, const ma_opt_t *opt);
int mahip_hits_cut_contained_finish(mahip_ctx_t *c, size_t *n_cut, uint32_t *n_seq_new);

int mahip_sub_upload(mahip_ctx_t *c, int slot, const ma_sub_t *sub, size_t n_sub);
int mahip_sub_download(mahip_ctx_t *c, int slot, ma_sub_t *sub, int squeezed); /* squeezed: compacted by the contained map */
int mahip_seqdel_download(mahip_ctx_t *c, uint8_t *del);                       /* per old read id, after contained */
int mahip_map_download(mahip_ctx_t *c, int32_t *map);                          /* old -> new id (-1 dropped) */
uint32_t mahip_n_seq_new(mahip_ctx_t *c);                                      /* reads left after contained (else n_seq) */
int mahip_survivors_download(mahip_ctx_t *c, uint32_t *old_ids);               /* [n_seq_new] new id -> old id */
size_t mahip_hits_live(mahip_ctx_t *c);
/* live hits, compacted, in the order ma_hit_sort + the order-preserving filters leave them in (hit.c:19-22, 162-258), ids renumbered
 * if contained has run; out must hold mahip_hits_live() */
int mahip_hits_download(mahip_ctx_t *c, ma_hit_t *out, size_t *n);

/* ---- string graph ---------------------------------------------------------------------------------- */
/* asm.c:9-39 ma_sg_gen (+ asg.c:72-80 asg_cleanup with the reference's arc order) from the resident hits.
 * use_sub: lengths from sub slot 0 (else seq_len).  seq_len/seq_del: optional host arrays indexed by the
 * CURRENT read numbering (needed when use_sub == 0; seq_del may be NULL). */
int mahip_sg_gen(mahip_ctx_t *c, const ma_opt_t *opt, int use_sub, const uint32_t *seq_len, const uint8_t *seq_del, uint32_t *n_arc);
/* per-symbol path: take a host graph (dense, sorted, indexed) */
int mahip_asg_upload(mahip_ctx_t *c, const asg_t *g);
/* asg.c:148-193 asg_arc_del_trans marking + asg_cleanup (symm is a separate call, as in the reference) */
int mahip_asg_del_trans(mahip_ctx_t *c, int fuzz, uint32_t *n_reduced);
/* asg.c:104-145 asg_arc_del_multi / asg_arc_del_asymm, each followed by asg_cleanup when it removed arcs */
int mahip_asg_symm(mahip_ctx_t *c, uint32_t *n_multi, uint32_t *n_asymm);
int mahip_asg_del_multi(mahip_ctx_t *c, uint32_t *n_multi);   /* asg.c:104-121 */
int mahip_asg_del_asymm(mahip_ctx_t *c, uint32_t *n_asymm);   /* asg.c:124-138 */
/* asg.c:83-101 asg_arc_del_short marking + cleanup (symm separate) */
int mahip_asg_del_short(mahip_ctx_t *c, float drop_ratio, uint32_t *n_short);
/* Renumber the device graph to the squeezed read ids (sdict.c:69-86 applied to the graph, as the reference has it from ma_sg_gen
 * on): a relabelling -- arc order and CSR positions are unchanged -- after which the cleaners and the unitig pass sweep the
 * surviving reads only.  No-op when no squeeze map is pending. */
int mahip_asg_squeeze(mahip_ctx_t *c);
/* Streams of inputs: hand the reduced graph to a SECOND context on the same device, so that the latency-bound rest of a batch (cleaners,
 * unitigs, downloads: ma_pipeline_tail_fetch on `to`, from another host thread) runs beside the next batch's hit passes on `from`.
 * `from` must hold a graph (after mahip_asg_del_trans / symm); it is squeezed first.  `to` receives the squeezed graph, the surviving reads'
 * intervals (sub slot 0) and their old ids -- O(survivors + arcs) bytes, device to device -- and answers the same queries a context answers
 * after ma_hit_contained + ma_sg_gen (mahip_n_seq_new, mahip_survivors_download, mahip_sub_download, the graph passes, mahip_ug_gen).
 * Returns when the copies are complete: `from` may be reused at once. */
int mahip_tail_handoff(mahip_ctx_t *from, mahip_ctx_t *to);
/* The order-dependent cleaners (asg.c:238-433) as a device fixpoint over versioned state (csrc/clean_core.h); each includes the
 * asg_cleanup the reference runs when something was cut.  Results equal the reference's sequential sweeps exactly. */
int mahip_asg_cut_tip(mahip_ctx_t *c, int max_ext, uint32_t *n_cut);                       /* asg.c:238-254 */
int mahip_asg_cut_internal(mahip_ctx_t *c, int max_ext, uint32_t *n_cut);                  /* asg.c:256-272 */
int mahip_asg_cut_biloop(mahip_ctx_t *c, int max_ext, uint32_t *n_cut);                    /* asg.c:274-306 */
int mahip_asg_pop_bubble(mahip_ctx_t *c, int max_dist, uint32_t *n_pop, uint32_t *n_tips); /* asg.c:412-433 (the graph must be symmetric) */
/* how many asg_pop_bubble calls of this context were run as the reference's sequential sweep on one lane (graphs that are not symmetric or not clean:
 * csrc/clean_core.h, ASSUMPTION; MA_BUBBLE_SEQ=1 forces it) */
uint32_t mahip_bubble_seq_sweeps(mahip_ctx_t *c);
/* What the LAST mahip_asg_cut_tip / _cut_internal / _cut_biloop / _pop_bubble call of this context did (host bookkeeping, read-only; the tests assert
 * from it that a case reached the tier, kernel form and sweep count it was built for).  n_iter: sweeps of the fixpoint, the one that found nothing
 * new included (0: the call returned before its first sweep -- no reads, no arcs, no bubble source).  Bubbles only: max_tier = the highest table
 * tier launched; n_src[t] = sources handed to tier t, summed over the sweeps; form[t] = the kernel form tier t last ran in (0: never launched);
 * seq_sweep: the call ended in the reference's sequential sweep on one lane (then the graph is that sweep's, whatever the fixpoint did before). */
enum { MAHIP_BUBBLE_TIERS = 5, MAHIP_BUBBLE_THREAD = 1, MAHIP_BUBBLE_WAVE_LDS = 2, MAHIP_BUBBLE_WAVE_HBM = 3 };
typedef struct { uint32_t n_iter, max_tier, seq_sweep, form[MAHIP_BUBBLE_TIERS]; uint64_t n_src[MAHIP_BUBBLE_TIERS]; } mahip_clean_info_t;
int mahip_clean_last(mahip_ctx_t *c, mahip_clean_info_t *out);
/* asm.c:121-210 ma_ug_gen on the device (csrc/ug.hip): unitigs of the current graph.  Counts: unitigs, reads on them, arcs
 * between unitig ends.  mahip_ug_download: per unitig {reads, length, start, end} (start == end == 0xffffffff: circular) and the
 * offset of its members; members = vertex << 32 | length to the next read; uarcs = the unitig arcs in push order (the
 * reference sorts them with its own sort afterwards, asm.c:208). */
int mahip_ug_gen(mahip_ctx_t *c, uint32_t *n_utg, uint32_t *n_members, uint32_t *n_uarc);
/* (a destination that is NULL is left out) */
int mahip_ug_download(mahip_ctx_t *c, uint32_t *u_n, uint32_t *u_len, uint32_t *u_start, uint32_t *u_end, uint32_t *u_off, uint64_t *members, asg_arc_t *uarcs);
/* asm.c:216-290 ma_ug_seq as a device byte gather (csrc/useq.hip).  Host reader (gzip, stdin, files outside the regular form below): it reads the sequence file and hands the bases of the
 * reads that sit on a unitig over in batches; a job copies `len` bases from the batch buffer to the unitig arena -- the first `len`
 * bases at src_off (forward) or the reverse complement of the last `len` of the src_len bases there (reverse). */
typedef struct { uint64_t src_off, dst_off; uint32_t src_len, len; uint32_t rev, pad; } mahip_useq_job_t;
int mahip_useq_begin(mahip_ctx_t *c, size_t arena_bytes);          /* arena of all unitig strings, filled with 'N' */
int mahip_useq_batch(mahip_ctx_t *c, const char *h_seq, size_t seq_bytes, const mahip_useq_job_t *h_jobs, size_t n_jobs);
int mahip_useq_end(mahip_ctx_t *c, char *h_arena);                 /* the arena back to the host; h_arena == NULL: no download, the finished arena stays in HBM until the next mahip_useq_begin (mahip_text_prepare_ug reads it) */
/* The reads file read on the device (csrc/useq.hip, replaces kseq.h:192-232 kseq_read + sdict.c sd_get + the copy loops of asm.c:262-284 for files in the
 * REGULAR FORM): the whole text goes to HBM, a newline census and a scan give every line its start, one pass over the lines checks the form, the wanted reads'
 * names go into a hash table that every record's name is looked up in, and the bases are copied from the text into the arena of mahip_useq_begin.
 * Regular form = the line index alone fixes the records, and kseq reads the same ones: no '\r' byte; no NUL byte (the reference's names are C strings, asm.c:266:
 * a NUL ends one); no line of 16 MiB or more inside a wrapped FASTA record (the placement sums 256 line lengths in 32 bits); first byte '>' (FASTA: every line that begins with '>' is
 * a header, no other non-empty line begins with '@' or '+', empty lines are skipped, sequences may be wrapped) or '@' (FASTQ: four lines a record -- '@' header,
 * a sequence line beginning with none of '>' '@' '+', a '+' line, a quality line of exactly the sequence's length); at most 2^32 - 1 lines.  Anything else comes
 * back as regular = 0 with a reason; that is not an error: the caller keeps its host reader (host/unitig_gfa.c). */
enum { MAHIP_FASTX_OK = 0, MAHIP_FASTX_CR, MAHIP_FASTX_FIRST_BYTE, MAHIP_FASTX_FASTA_LINE_START, MAHIP_FASTX_FASTQ_SHAPE, MAHIP_FASTX_FASTQ_QUAL_LEN, MAHIP_FASTX_TOO_MANY_LINES,
       MAHIP_FASTX_NOMEM, MAHIP_FASTX_SHORT_READ, MAHIP_FASTX_NOT_PLAIN, MAHIP_FASTX_FORCED, MAHIP_FASTX_NUL_BYTE, MAHIP_FASTX_LONG_LINE };
enum { MAHIP_FASTX_FASTA = 1, MAHIP_FASTX_FASTQ = 2 };
typedef struct {
	int format;               /* MAHIP_FASTX_FASTA / _FASTQ by the first byte, 0: neither */
	uint64_t n_lines;         /* a last line without '\n' counts */
	uint64_t n_records;       /* FASTA: header lines; FASTQ: n_lines / 4 */
	uint64_t n_cr;            /* '\r' bytes */
	int regular, reason;      /* regular = 1 <=> reason == MAHIP_FASTX_OK */
} mahip_fastx_info_t;
int mahip_fastx_load_mem(mahip_ctx_t *c, const void *text, size_t nbytes);  /* nbytes > 0 */
int mahip_fastx_load_fd(mahip_ctx_t *c, int fd, size_t nbytes);             /* bytes [0,nbytes) of an open plain file; 1: no device memory for it, -1: error */
int mahip_fastx_index(mahip_ctx_t *c, mahip_fastx_info_t *info);            /* returns 0 with reason _NOMEM when the index does not fit */
int mahip_fastx_release(mahip_ctx_t *c);                                    /* the text, the index and the lookup tables go back to the pool */
const char *mahip_fastx_reason_name(int reason);
/* for stage tests: out[0 .. n_lines] = offset of the first byte of every line, out[n_lines] = nbytes (+ 1 when the last line has no '\n'): line i is bytes
 * [out[i], out[i+1] - 1); and, for a regular text, where every record's name stands in it (n_records entries each) */
int mahip_fastx_line_starts(mahip_ctx_t *c, uint64_t *out);
int mahip_fastx_name_spans(mahip_ctx_t *c, uint64_t *off, uint32_t *len);
/* A read that sits on a unitig: its name (bytes [name_off, name_off + name_len) of `names`, exact byte string as sd_get compares it, sdict.c), where its
 * `len` bases go, the strand, and the kept interval [s, e) of the read they are taken from (whole = 1: the whole record, as ma_ug_seq without `sub`).
 * Forward: the first len bases of the interval; reverse: the reverse complement of its last len (asm.c:275-283). */
typedef struct { uint64_t dst_off, name_off; uint32_t name_len, len, s, e, rev, whole; } mahip_useq_want_t;
/* between mahip_useq_begin and mahip_useq_end, on a regular text: looks every record's name up (names are distinct; a name the file carries more than once
 * takes its LAST record, as the reference's loop does) and copies.  n_matched = wanted reads found, n_dup = matching records beyond the first of a name, n_short =
 * matching records with fewer bases than the placement needs (e, or len with whole).  n_short > 0: NOTHING is placed -- the caller falls back to its host reader,
 * which keeps the reference's behaviour for such files.  laps_ms (optional): wall time of lookup and placement (the latter costs a stream sync). */
int mahip_useq_place_text(mahip_ctx_t *c, const mahip_useq_want_t *wanted, size_t n_wanted, const char *names, size_t name_bytes,
                          uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms);
/* What the LAST ma_ug_seq of this context did (host bookkeeping, noted by host/unitig_gfa.c through mahip_useq_note; the tests assert from it that an input reached
 * the reader it was built for): reader 1 = host, 2 = device; reason: why the host reader ran (MAHIP_FASTX_*). */
enum { MAHIP_USEQ_HOST = 1, MAHIP_USEQ_DEVICE = 2, MAHIP_USEQ_STREAM = 3 }; /* 3: the streamed device reader below; reason = why it handed the rest of the input to the host reader (OK: it did not) */
typedef struct { int reader, reason, format; uint64_t n_records, n_matched, n_dup, n_short; } mahip_useq_info_t;
void mahip_useq_note(mahip_ctx_t *c, const mahip_useq_info_t *in);
int mahip_useq_last(mahip_ctx_t *c, mahip_useq_info_t *out);
/* The reads file read on the device A PIECE AT A TIME (csrc/useq.hip): for input that cannot lie in HBM whole or cannot be opened twice -- gzip through
 * zlib, stdin, a FIFO.  The caller feeds pieces of WHOLE LINES in input order; the device keeps one WINDOW = the carry (the trailing bytes of the window before
 * that did not yet form a complete record; it never leaves the device) + the piece, consumes the complete records of the window and carries the rest:
 *   FASTQ  with L newline-terminated lines in the window the records are lines 0 .. 4*floor(L/4) - 1 (kseq.h:222-230: header, ONE sequence line, '+', ONE quality
 *          line of the sequence's length -- the form the check below verifies);
 *   FASTA  everything in front of the window's last header line: the last record may go on in the next piece (kseq.h:209-213 reads sequence lines until the next
 *          '>'), so it is always carried;
 *   the last window is consumed whole; its final line may lack the '\n' (kseq.h:139-144); a FASTQ last window whose line count is no multiple of 4 is FASTQ_SHAPE.
 * The format is fixed by the first byte of the INPUT (kseq.h:197-199 scans to the first '>' or '@'); every later window is checked in that format.  Every window
 * gets a verdict over its complete records BEFORE it touches the arena -- the checks of the regular form above ('\r', NUL, FASTA line starts, FASTQ shape and
 * quality length, LONG_LINE) and SHORT_READ (a matching record with fewer bases than its placement, asm.c:279-285).  A verdict other than OK ends the stream:
 * windows 0 .. k-1 stay placed, window k places nothing, and the caller's host reader takes over from the first byte of window k, which is a record boundary where
 * kseq's state is `last_char == 0` (FASTQ, kseq.h:229) or "just consumed the next header's '>'" (FASTA, kseq.h:214) -- a fresh reader that scans to the first
 * '>' / '@' (kseq.h:197) continues identically.  A name the input carries more than once takes its LAST record (asm.c:262-284 overwrites): inside a window by the
 * record number, across windows by stream order; n_matched counts distinct names, n_dup matching records beyond the first of a name, over the whole stream.
 * Per window the cost follows the window, never the wanted list: the table over the wanted names is built once (begin), the probe appends the wanted reads that
 * matched to a list and the placement runs one block per entry, which also clears the entry's slot of the per-wanted record array for the next window. */
typedef struct {
	int reason;                /* MAHIP_FASTX_*; anything but OK: nothing of this window was placed and the stream takes no more pieces */
	uint64_t n_records;        /* complete records of the window */
	uint64_t bytes_consumed;   /* bytes of the window in front of the carry (0 with a reason) */
	uint64_t carry_bytes;      /* bytes kept for the next window */
	uint64_t n_placed;         /* wanted reads this window placed (the length of its match list) */
} mahip_useq_stream_verdict_t;
typedef struct {
	int format;                /* MAHIP_FASTX_FASTA / _FASTQ by the first byte of the input; 0: no byte yet, or neither */
	uint64_t n_pieces;         /* pieces taken, empty ones and a refused one included */
	uint64_t n_records, n_matched, n_dup, n_short; /* over the windows that were placed (n_short: of the refused window) */
	uint64_t n_jobs;           /* sum of the match-list lengths = blocks of the placement launched */
	uint64_t max_carry;        /* the largest carry, bytes */
	uint32_t n_window_grow;    /* times the window buffer was replaced by a larger one (the first buffer replaces none) */
	int refused_reason;        /* MAHIP_FASTX_* of the refused piece */
	int64_t refused_piece;     /* -1: none */
	double laps_ms[4];         /* wall time so far: upload (carry move included), line index + prefix + form, lookup, placement */
} mahip_useq_stream_report_t;
int mahip_useq_stream_begin(mahip_ctx_t *c, const mahip_useq_want_t *wanted, size_t n_wanted, const char *names, size_t name_bytes); /* between mahip_useq_begin and mahip_useq_end; asm.c:248-260 (where every read lands) as the wanted list */
int mahip_useq_stream_piece_mem(mahip_ctx_t *c, const void *text, size_t nbytes, int last, mahip_useq_stream_verdict_t *v); /* asm.c:262-284 + kseq.h:192-232 on the window's records; whole lines, only the last piece may lack '\n'; nbytes may be 0 */
int mahip_useq_stream_window_download(mahip_ctx_t *c, void *dst, uint64_t *nbytes); /* after a verdict != OK: the bytes of the refused window (carry + piece); dst == NULL: only the size */
int mahip_useq_stream_end(mahip_ctx_t *c);   /* waits for the last placement; the arena is mahip_useq_end's */
int mahip_useq_stream_abort(mahip_ctx_t *c); /* legal without a stream */
int mahip_useq_stream_last(mahip_ctx_t *c, mahip_useq_stream_report_t *out); /* valid from begin until the next begin */
/* The placement plan on the device (csrc/useq.hip): asm.c:248-260 -- where every unitig's string starts in the arena and where every read that sits
 * on a unitig lands on it -- plus the wanted table of the device readers (host/unitig_gfa.c: ug_seq_wanted), from the unitigs mahip_ug_gen left in the context, the
 * names of mahip_text_names and the kept intervals of slot 0, in the numbering mahip_text_prepare_ug uses.  No member word comes down.
 *   uoff[i]   = sum over j < i of (u_len[j] + 1), 64 bits (asm.c:250: `tot`, one terminator per string); arena_bytes = uoff[n_utg]
 *   per read  : utg, ori = m >> 32 & 1, len = (uint32_t)m, start = the sum mod 2^32 of the low words of the members in front of it on its unitig (asm.c:252-258,
 *               the reference's uint32_t l: the same number the `a` lines print, csrc/text_core.h: tc_ug_member_start); a read on no unitig has len 0
 *   wanted    : the reads with len != 0 and a name that is not empty, in ascending read id: dst_off = uoff[utg] + start (64 bits), len, rev = ori, whole = !have_sub,
 *               s / e = the kept interval (0 without), name_off / name_len = the read's name IN THE BLOB OF mahip_text_names -- the names are not copied; the table
 *               is valid until the next mahip_text_names, mahip_ug_gen or plan of the context.
 * A read that is a member more than once makes the reference assert (asm.c:255); here the plan refuses (MULTI) and the caller keeps its host plan.
 * Returns 0 with info->road = DEVICE; or 0 with road = HOST and a reason: no plan is held then, and nothing else in the context -- arena, loaded text, the tables of
 * the host-table entries -- has changed; or -1 (error: a member names a read outside the dictionary, a HIP error). */
enum { MAHIP_PLAN_ROAD_HOST = 1, MAHIP_PLAN_ROAD_DEVICE = 2 };
enum { MAHIP_PLAN_OK = 0, MAHIP_PLAN_NO_UG,  /* the context holds no unitigs (mahip_ug_gen has not run, or found none) */
       MAHIP_PLAN_NO_NAMES,                  /* mahip_text_names has not described the reads the members name */
       MAHIP_PLAN_MULTI,                     /* a read is a member more than once */
       MAHIP_PLAN_NOMEM,                     /* no device memory for the plan */
       MAHIP_PLAN_FORCED };                  /* MA_USEQ_PLAN_HOST=1 */
typedef struct { uint32_t utg, start, len, ori; } mahip_useq_place_t; /* one per read: host/unitig_gfa.c: utg_place_t with its fields as words */
typedef struct {
	int road, reason;
	uint64_t n_utg, n_members, n_reads;
	uint64_t n_wanted;       /* entries of the wanted table */
	uint64_t name_bytes;     /* bytes of the wanted reads' names */
	uint64_t blob_bytes;     /* bytes of the blob the table's name_off point into (mahip_useq_plan_download: `names`) */
	uint64_t arena_bytes;    /* uoff[n_utg] */
	uint64_t n_multi;        /* members that found their read taken already */
	uint64_t uoff_tiles;     /* tiles of the 64-bit scan (more than one: block sums, their scan, the down sweep) */
	double ms;               /* wall time of the plan, its one wait for the device included */
} mahip_useq_plan_info_t;
int mahip_useq_plan(mahip_ctx_t *c, int have_sub, mahip_useq_plan_info_t *info);
int mahip_useq_plan_last(mahip_ctx_t *c, mahip_useq_plan_info_t *info); /* the info of the last plan, refused ones included */
const char *mahip_useq_plan_reason_name(int reason);
/* stage entry (tests), the counterpart of mahip_text_format_ug_mem: hand-made unitigs (u_n members each, back to back in `members`), n_seq names (blob / off as
 * mahip_text_names takes them, which it calls; blob == 0: NO_NAMES) and kept intervals (ma_sub_t, n_seq of them, or 0) from host memory.  Allocates no arena, so
 * u_len may be anything.  Whatever MA_TEXT_DEVICE says; MA_USEQ_PLAN_HOST=1 refuses here too. */
int mahip_useq_plan_mem(mahip_ctx_t *c, uint32_t n_utg, const uint32_t *u_n, const uint32_t *u_len, const uint64_t *members, uint32_t n_seq, const char *blob, const uint64_t *off,
                        const void *sub, mahip_useq_plan_info_t *info);
/* the plan to the host: uoff[n_utg + 1], pl[n_reads], want[n_wanted], names[blob_bytes]; a destination that is NULL is left out.  For the host reader, which needs
 * pl and uoff (asm.c:262-284), for ma_ug_seq_fetch, which cuts the arena with uoff, and for the tests. */
int mahip_useq_plan_download(mahip_ctx_t *c, uint64_t *uoff, mahip_useq_place_t *pl, mahip_useq_want_t *want, char *names);
/* the planned forms: mahip_useq_begin with the plan's arena_bytes; mahip_useq_place_text and mahip_useq_stream_begin with the plan's wanted table, which is on the
 * device already (asm.c:248-260 as that table; everything behind the upload is the host-table entries' own code).  -1 without a plan, or when the arena is not the
 * plan's (mahip_useq_begin_planned), or when an entry of the table reaches outside it. */
int mahip_useq_begin_planned(mahip_ctx_t *c);
int mahip_useq_place_text_planned(mahip_ctx_t *c, uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms);
int mahip_useq_stream_begin_planned(mahip_ctx_t *c);
/* ---- bgzip-compressed (BGZF) input inflated on the device (csrc/xfer.hip: k_bgzf_inflate, csrc/inflate_core.h; the member walk: host/ingest_gpu.c).
 * A BGZF file is a chain of gzip members of at most 64 KiB of text each, every one with its compressed size in a `BC` extra subfield and its inflated size in
 * its trailer: the host walks the chain once (one small read per member) into a table -- where each member's deflate bytes lie, its CRC and ISIZE, and where
 * its text goes (out_off: a 64-bit exclusive prefix sum of ISIZE, the text of a big overlap file exceeds 4 GiB) -- the compressed file goes to HBM as it is, one
 * wave inflates one member into its slice of the text buffer, and a second pass checks every member's CRC-32.  Afterwards the text lies where
 * mahip_paf_load_fd / mahip_fastx_load_fd would have put it.  Everything that keeps the device from doing this comes back as a `reason`, which is not an error:
 * nothing is loaded then and the caller inflates with zlib, as it does for plain gzip and stdin.
 *   the walk's refusals  NOT_BGZF: the first member is not a BGZF member (plain gzip: no extra field, or none with `BC`); NO_BC: a later member without `BC`;
 *                        PAST_END: a member (or its header) runs past the end of the file, or is too short for its header and trailer; TRAILING: bytes behind the
 *                        chain that do not begin a gzip member; BAD_FLG: a header flag that adds a field the walk does not skip (FNAME, FCOMMENT, FHCRC, reserved);
 *                        ISIZE: a member claims more than 65536 bytes of text
 *   the kernel's statuses (of the first member that has one; csrc/inflate_core.h)  BAD_BTYPE: block type 3; STORED_LEN: LEN != ~NLEN; BAD_LENGTHS: over-subscribed
 *                        or otherwise invalid code lengths; BAD_SYMBOL; DIST_TOO_FAR: a distance reaches in front of the member's own output; OUT_OVERFLOW: more
 *                        output than ISIZE; IN_EXHAUSTED: the deflate bytes end early; OUT_SHORT: less output than ISIZE; CRC: the text's CRC-32 is not the trailer's
 *   NOMEM: no device memory for the compressed bytes, the table or (target NONE, FASTX) the text; NOT_SEEKABLE: not a regular file; FORCED: MA_BGZF_HOST is set;
 *   EMPTY: target FASTX and no text at all (the reads-file reader has nothing to index, as for an empty plain file) */
enum { MAHIP_BGZF_OK = 0, MAHIP_BGZF_NOT_BGZF, MAHIP_BGZF_NO_BC, MAHIP_BGZF_PAST_END, MAHIP_BGZF_TRAILING, MAHIP_BGZF_BAD_FLG, MAHIP_BGZF_ISIZE,
       MAHIP_BGZF_BAD_BTYPE, MAHIP_BGZF_STORED_LEN, MAHIP_BGZF_BAD_LENGTHS, MAHIP_BGZF_BAD_SYMBOL, MAHIP_BGZF_DIST_TOO_FAR, MAHIP_BGZF_OUT_OVERFLOW, MAHIP_BGZF_IN_EXHAUSTED,
       MAHIP_BGZF_OUT_SHORT, MAHIP_BGZF_CRC, MAHIP_BGZF_NOMEM, MAHIP_BGZF_NOT_SEEKABLE, MAHIP_BGZF_FORCED, MAHIP_BGZF_EMPTY };
enum { MAHIP_BGZF_HOST = 1, MAHIP_BGZF_DEVICE = 2 };
enum { MAHIP_BGZF_PAF = 1, MAHIP_BGZF_FASTX = 2 }; /* target: whose text buffer the members are inflated into */
typedef struct {
	uint64_t n_members, n_empty;           /* members of the chain; those with ISIZE == 0 (the end-of-file marker is one) */
	uint64_t n_stored, n_fixed, n_dynamic; /* deflate blocks by type, over all members (counted by the kernel: 0 when it did not run) */
	uint64_t comp_bytes, text_bytes;       /* the file; the sum of ISIZE */
	int reader, reason;                    /* MAHIP_BGZF_DEVICE <=> reason == MAHIP_BGZF_OK */
	int64_t first_bad_member;              /* the member the reason is about (walk: where it stopped; kernel: the first member with a status), else -1 */
	double laps_ms[4];                     /* walk, upload, inflate, CRC */
} mahip_bgzf_info_t;
/* one row of the block table (host/ingest_gpu.c: ma_bgzf_walk makes it, the kernels read it) */
typedef struct { uint64_t in_off, out_off; uint32_t in_len, isize, crc, pad; } mahip_bgzf_member_t;
/* 0 with info->reason == MAHIP_BGZF_OK: the context is in the state mahip_paf_load_fd (target PAF: the same reservation, the same padding, MA_PAF_MAX_BYTES
 * applies to the inflated size) or mahip_fastx_load_fd (target FASTX) leaves, the compressed bytes and the table are back in the pool.  0 with another reason:
 * nothing is loaded, take the host road.  -1: a real error (a read error, a HIP error, what mahip_paf_load_fd itself fails on). */
int mahip_bgzf_load_fd(mahip_ctx_t *c, int fd, size_t nbytes, int target, mahip_bgzf_info_t *info);
int mahip_bgzf_load_mem(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, mahip_bgzf_info_t *info);
/* for stage tests: a BGZF image in host memory -> its text in host memory (out_cap >= info->text_bytes, else -1); nothing stays loaded */
int mahip_bgzf_inflate_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, void *out, size_t out_cap, mahip_bgzf_info_t *info);
/* Sharded ingest of a BGZF overlap file (host/ingest_sharded.c): rank `rank` of `world` inflates only the members that hold ITS range of the text,
 * the same range host/ingest_sharded.c cuts out of a plain file.  With T = the chain's text_bytes and nom(g) = T g / world (64-bit), the range is [beg, end) =
 * [ls(nom(rank)), ls(nom(rank + 1))), end = T on the last rank, where ls(a) = 0 for a <= 0, T for a >= T, else the byte behind the first '\n' at a position
 * >= a - 1 (T when there is none): a function of the text alone, so two ranks compute the border between them independently and agree.  The host walks the
 * WHOLE chain (the table is what makes a member range addressable: that lap does not shrink with `world`); uploaded and inflated are the members from the one
 * that holds byte max(nom(rank) - 1, 0) (first_member; empty members in front of it are skipped) through the one that holds byte nom(rank + 1) - 1, plus
 * MAHIP_BGZF_RANGE_AHEAD members; k_text_first_nl finds both borders in the inflated text.  A border whose newline is not there (a line that runs across more
 * members than the look-ahead) is looked for again after the next batch of members has been inflated and checked: MAHIP_BGZF_RANGE_AHEAD members, twice as many
 * each further round, to the end of the chain (where the border is T): n_rounds <= log2(n_members) + 1 launches' worth, no wait inside a kernel.
 * MAHIP_BGZF_RANGE_AHEAD = 1: a PAF line is a few hundred bytes and a member holds up to 64 KiB of text, so a border's newline lies in the member of its
 * nominal position or, when that member ends inside the line, in the next one; one member more costs a rank about 16 KiB of upload and one wave, a round
 * costs an upload, two launches and three waits for the stream.  Only a line of more than a member's text needs a round. */
#define MAHIP_BGZF_RANGE_AHEAD 1
typedef struct {
	uint64_t text_bytes;                       /* T: the inflated size of the whole file */
	uint64_t beg, end;                         /* this rank's text, positions in the inflated file */
	uint64_t first_member, n_members_inflated; /* members [first_member, first_member + n_members_inflated) of the chain were uploaded, inflated and CRC-checked
	                                            * (none when nom(rank + 1) = 0); first_member = n_members when no member holds byte max(nom(rank) - 1, 0) (T = 0) */
	uint64_t comp_bytes_uploaded;              /* from the first of them's deflate bytes to the last one's */
	int n_rounds;                              /* extension rounds */
} mahip_bgzf_range_t;
/* target PAF; NOT collective (the range is a function of the file, rank and world alone).  0 with info->reason == MAHIP_BGZF_OK: the context is in the state
 * mahip_paf_load_fd_range(c, plain, range->beg, range->end - range->beg) leaves on the inflated file (the reservation of end - beg bytes, which is what
 * MA_PAF_MAX_BYTES counts, the padding), everything but the text is back in the pool.  info as for mahip_bgzf_load_fd: n_members, n_empty, text_bytes and
 * comp_bytes are the whole chain's, the block counts and laps_ms (walk, upload, inflate, CRC; the last three summed over the rounds) this rank's,
 * first_bad_member counts in the whole chain.  Other return values as mahip_bgzf_load_fd: another reason is no error, nothing stays loaded.  Prints nothing. */
int mahip_bgzf_load_fd_range(mahip_ctx_t *c, int fd, size_t nbytes, int rank, int world, mahip_bgzf_range_t *range, mahip_bgzf_info_t *info);
/* for stage tests: a BGZF image in host memory -> the rank's text in host memory (out_cap >= range->end - range->beg, else -1) and its range; nothing stays loaded */
int mahip_bgzf_range_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, int rank, int world, void *out, size_t out_cap, mahip_bgzf_range_t *range, mahip_bgzf_info_t *info);
/* for stage tests: the search alone (csrc/xfer.hip: k_text_first_nl).  *pos = the position of the first '\n' among the bytes [from, to) of the DEVICE text
 * d_text, or all ones when there is none (or to <= from).  Any byte positions: nothing outside [from, to) is read.  Waits for the stream. */
int mahip_text_first_nl(mahip_ctx_t *c, const void *d_text, uint64_t from, uint64_t to, uint64_t *pos);
int mahip_bgzf_last(mahip_ctx_t *c, mahip_bgzf_info_t *out); /* what the context's last BGZF load (or mahip_bgzf_note) decided */
void mahip_bgzf_note(mahip_ctx_t *c, const mahip_bgzf_info_t *in); /* a caller that did not get as far as a load (MA_BGZF_HOST) says so */
const char *mahip_bgzf_reason_name(int reason);
/* ---- plain gzip input (one member, one deflate stream: what `gzip -1` writes; concatenated members: further below) inflated on the device (csrc/xfer.hip: k_gz_*, csrc/gzip_core.h).
 * The host reads the member's header and trailer; the compressed file goes to HBM as it is; its payload is cut into chunks of `chunk` bytes.  k_gz_sync_count:
 * one wave per chunk looks in its own bits for the first dynamic-block header that holds and that a trial decode of the block confirms (chunk 0 starts at bit
 * 0), then decodes on WITHOUT output, summing the output length, to the first dynamic block start in a later chunk, or to the end of the stream: one row per
 * chunk.  The host follows the rows from chunk 0 (`end_bit` of one must be `sync_bit` of the chunk it falls into): the chain's items, their output offsets,
 * the text size.  k_gz_decode: one wave per item writes 16-bit symbols (a byte, or a cell of the unknown 32 KiB in front of the item); k_gz_windows: one
 * workgroup a member makes every item's window from the one before it; k_gz_resolve writes the text, k_gz_crc checks it against the trailer.  Every refusal is a
 * `reason`, not an error: nothing is loaded and the caller inflates with zlib.
 *   BAD_HEADER: not a gzip member, CM != 8, a reserved flag, an extra field with a `BC` subfield, or too short for header and trailer;
 *   MULTI_MEMBER: the stream's final block does not end 8 bytes in front of the end of the file (a second member, trailing bytes);
 *   NO_SYNC: an item ran over more than GZ_SPAN_MAX (16) whole chunks without reaching its end; SYNC_MISMATCH: an item ends in a chunk whose own first
 *   block start is another bit (a false candidate stood in front of the true one); ISIZE: the items' total is not the trailer's ISIZE (mod 2^32);
 *   BAD_BTYPE .. OUT_SHORT: the status of an item on the chain, as for BGZF; CRC; NOMEM, NOT_SEEKABLE, FORCED (the switch is off), EMPTY: as for BGZF. */
enum { MAHIP_GZIP_OK = 0, MAHIP_GZIP_BAD_HEADER, MAHIP_GZIP_MULTI_MEMBER, MAHIP_GZIP_NO_SYNC, MAHIP_GZIP_SYNC_MISMATCH, MAHIP_GZIP_ISIZE,
       MAHIP_GZIP_BAD_BTYPE, MAHIP_GZIP_STORED_LEN, MAHIP_GZIP_BAD_LENGTHS, MAHIP_GZIP_BAD_SYMBOL, MAHIP_GZIP_DIST_TOO_FAR, MAHIP_GZIP_OUT_OVERFLOW, MAHIP_GZIP_IN_EXHAUSTED,
       MAHIP_GZIP_OUT_SHORT, MAHIP_GZIP_CRC, MAHIP_GZIP_NOMEM, MAHIP_GZIP_NOT_SEEKABLE, MAHIP_GZIP_FORCED, MAHIP_GZIP_EMPTY,
       MAHIP_GZIP_TOO_MANY_CANDIDATES /* the *_members forms: the member scan found more candidate positions than its list holds */ };
#define MAHIP_GZIP_CHUNK_DEFAULT ((size_t)1 << 20) /* bytes of payload per chunk; MA_GZIP_CHUNK (a power of two, 1024 .. 16 MiB) overrides it */
typedef struct {
	uint64_t comp_bytes, text_bytes;       /* the file; the items' total output */
	uint64_t chunk, n_chunks, n_synced, n_items; /* chunk size; chunks; those that found a start (chunk 0 included); items on the chain */
	uint64_t n_stored, n_fixed, n_dynamic; /* deflate blocks by type over the chain (counted by k_gz_decode: 0 when it did not run) */
	int reader, reason;                    /* MAHIP_BGZF_HOST | MAHIP_BGZF_DEVICE; MAHIP_BGZF_DEVICE <=> reason == MAHIP_GZIP_OK */
	int64_t first_bad_item;                /* the chain item (its number on the chain) the reason is about, else -1 */
	double laps_ms[6];                     /* upload, sync + count, decode, windows, resolve, CRC */
} mahip_gzip_info_t;
/* one row per chunk, as k_gz_sync_count leaves it; bits count from the first bit of the payload */
#define MAHIP_GZIP_SAW_FINAL 1u
#define MAHIP_GZIP_ON_CHAIN 2u
typedef struct {
	int64_t sync_bit;          /* where the chunk's item starts; -1: no start found (no item) */
	uint64_t end_bit, out_len; /* where it stopped; the bytes it inflates to */
	uint32_t status, flags;    /* 0 or the item's status as a MAHIP_GZIP_* reason; MAHIP_GZIP_SAW_FINAL, MAHIP_GZIP_ON_CHAIN */
} mahip_gzip_item_t;
/* target MAHIP_BGZF_PAF | MAHIP_BGZF_FASTX, return values and what is left loaded: as mahip_bgzf_load_fd.  chunk 0: MA_GZIP_CHUNK, else the default. */
int mahip_gzip_load_fd(mahip_ctx_t *c, int fd, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info);
int mahip_gzip_load_mem(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info);
/* for stage tests: image in host memory -> text in host memory (out_cap >= info->text_bytes, else -1); nothing stays loaded */
int mahip_gzip_inflate_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, size_t chunk, void *out, size_t out_cap, mahip_gzip_info_t *info);
int mahip_gzip_last(mahip_ctx_t *c, mahip_gzip_info_t *out);
void mahip_gzip_note(mahip_ctx_t *c, const mahip_gzip_info_t *in);
const char *mahip_gzip_reason_name(int reason);
/* the rows of the context's last plain-gzip load (n_chunks of them; none when it stopped at the header); valid until the next load.  Returns the number
 * of rows copied (at most cap). */
uint64_t mahip_gzip_items_download(mahip_ctx_t *c, mahip_gzip_item_t *out, uint64_t cap);
/* ---- concatenated gzip members (`cat a.gz b.gz`; what zlib's gzread reads as one text).  The three entry points above keep their contract: one member, and
 * MULTI_MEMBER otherwise.  The *_members forms take the same arguments and inflate every member into ONE text:
 *   k_gz_member_scan   every byte position behind the first header whose bytes read 1f 8b 08 and a FLG with bits 5..7 clear is a CANDIDATE (a list of at most
 *                      `cand_cap` positions; more: TOO_MANY_CANDIDATES).  The host sorts the list and reads a header at each one; a candidate whose header does
 *                      not parse is dropped.  False candidates are expected (a stored block may hold any bytes) and cost nothing: the chain never visits them.
 *   k_gz_heads         one wave per surviving candidate decodes, counting, from the first bit behind its header -- as k_gz_sync_count does for chunk 0 -- to the
 *                      first dynamic block start in a later chunk, or to BFINAL: one row per candidate (a HEAD ITEM; it may end in the chunk it starts in).
 *   the chain          where a member's final block ends (byte-aligned) + 8 is the end of the file or a position q.  If q is a candidate with a head row the
 *                      trailer at q - 8 closes the member (ISIZE against the member's own total) and the chain goes on with q's head row; else MULTI_MEMBER:
 *                      trailing bytes that begin no member this reader takes (zlib has its own rules for those and stays the one that applies them).
 *   history            a distance may not reach in front of its own member: DIST_TOO_FAR, as zlib fails on it.  k_gz_windows runs one workgroup per MEMBER.
 *   CRC                k_gz_crc works on pieces that never straddle a member; every member's CRC is compared with its own trailer.
 * A member without text (`gzip < /dev/null`) is legal and contributes nothing.  Chunks, bits and rows count from the first bit behind the FIRST member's header,
 * as above; headers and trailers of later members lie among the chunks' bytes. */
typedef struct {
	uint64_t n_members, n_candidates, n_heads; /* members on the chain (the one a refusal is about included); candidates the scan found; those with a header that parses */
	int64_t bad_member;                        /* the member (its number in the file, from 0) the reason is about, else -1 */
	uint64_t cand_cap;                         /* the capacity of the candidate list of this load */
	double laps_ms[2];                         /* the member scan (with the headers read on the host); the head items */
} mahip_gzip_members_info_t;
typedef struct {
	uint64_t comp_off, hdr_len;  /* where the member starts in the file; its header's length */
	uint64_t text_off, text_len; /* where its text lies in the whole text */
	uint32_t crc, isize;         /* its trailer (zero for a member the chain did not close) */
	uint64_t n_items;            /* chain items of this member */
} mahip_gzip_member_t;
#define MAHIP_GZIP_CAND_CAP_DEFAULT ((size_t)1 << 16) /* MA_GZIP_CAND_CAP overrides it (tests) */
int mahip_gzip_load_fd_members(mahip_ctx_t *c, int fd, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info);
int mahip_gzip_load_mem_members(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info);
int mahip_gzip_inflate_mem_members(mahip_ctx_t *c, const void *comp, size_t ncomp, size_t chunk, void *out, size_t out_cap, mahip_gzip_info_t *info);
/* the member facts of the context's last plain-gzip load (all zero, bad_member -1, after a load through the one-member entry points) */
int mahip_gzip_members_last(mahip_ctx_t *c, mahip_gzip_members_info_t *out);
/* one row per member of the last load, in file order; returns the number of rows copied (at most cap) */
uint64_t mahip_gzip_members_download(mahip_ctx_t *c, mahip_gzip_member_t *out, uint64_t cap);
uint32_t mahip_asg_n_arc(mahip_ctx_t *c);
/* how many device-wide scans (csrc/scan.hip) of this context, since it was created, took each form: one tile (k_scan_down alone, n <= 2048), the chained
 * launch (k_scan_chain, up to 256 tiles = 524 288 elements), reduce / scan of the tile sums / downsweep (k_scan_reduce, above).  Host bookkeeping only. */
enum { MAHIP_SCAN_ONE_TILE = 0, MAHIP_SCAN_CHAINED = 1, MAHIP_SCAN_THREE_PHASE = 2 };
void mahip_scan_forms(mahip_ctx_t *c, uint64_t out[3]);
/* for stage tests: the device-wide exclusive prefix sum (mod 2^32) of d_in[0 .. n) -> d_out[0 .. n), queued on the context's stream.  d_out may equal d_in
 * (in place; no other overlap); d_total may be NULL, else the sum of all n elements is written there (0 for n = 0).  PRECONDITION: d_in and d_out are 16-byte
 * aligned (full groups of eight elements are moved as two 16-byte words).  Nothing at or behind element n is written. */
int mahip_scan_u32(mahip_ctx_t *c, const uint32_t *d_in, uint32_t *d_out, size_t n, uint32_t *d_total);
/* iterations of the inner loop of asg_arc_del_trans (asg.c:169) in the last reduction this context ran, counted on the device: SURVEY 8(d) prices the
 * reduction at 16 (A + I) bytes (bench.py: roofline.reduce_group) */
uint64_t mahip_asg_trans_inner(mahip_ctx_t *c);
/* fills g (arc/seq/idx malloc'ed, is_srt=1) in the squeezed numbering */
int mahip_asg_download(mahip_ctx_t *c, asg_t *g);

/* ---- building blocks of the sharded multi-GPU mode ---------------------------------------------------
 * One context per GPU owns the hits whose query id lies in its read range (mahip_set_shard).  Passes that read
 * another read's sub/flags need the complete read-indexed arrays, so the caller exchanges them between the
 * split halves below (host/sharded.c: RCCL all-gather / max all-reduce on the context's stream);
 * the arcs are exchanged once, before the transitive reduction. */
#define MAHIP_BUF_SUB0  0   /* uint2 [n_seq] */
#define MAHIP_BUF_SUB1  1
#define MAHIP_BUF_RCONT 2   /* u8 [n_seq] contained flags   (hit.c:234-235) */
#define MAHIP_BUF_RUSED 3   /* u8 [n_seq] touched-by-a-hit  (hit.c:24-36) */
#define MAHIP_BUF_SDEL  4   /* u8 [n_seq] seq.del           (asm.c:27-34) */
/* device-to-device copies of elements [first, first+count) out of / into one of the arrays above */
int mahip_copy_out(mahip_ctx_t *c, int which, void *d_dst, size_t first, size_t count);
int mahip_copy_in(mahip_ctx_t *c, int which, const void *d_src, size_t first, size_t count);
/* hit.c:225-256 split at the point where the flags must be complete */
int mahip_hits_contained_flags(mahip_ctx_t *c, const ma_opt_t *opt);
int mahip_hits_contained_finish(mahip_ctx_t *c, const uint8_t *seq_del, uint32_t *n_seq_new, size_t *n_live);
/* asm.c:9-39 split at the point where seq.del must be complete */
int mahip_sg_flags(mahip_ctx_t *c, const ma_opt_t *opt, int use_sub, const uint32_t *seq_len, const uint8_t *seq_del);
int mahip_sg_finish(mahip_ctx_t *c, uint32_t *n_arc);
/* local sorted arcs as packed rows {u, v, len, ol|del<<31} (16 B each) */
int mahip_asg_export_rows(mahip_ctx_t *c, void *d_dst);
/* replace the graph by the concatenation of n_ranks blocks of rows (block r holds counts[r] rows at d_src + r*stride rows) */
int mahip_asg_import_rows(mahip_ctx_t *c, const void *d_src, const uint32_t *counts, int n_ranks, size_t stride);
/* Tie repair on shards: after the arc exchange every rank holds the whole sorted graph and its tie census
 * (mahip_tie_stats).  With tie groups: (1) mahip_sg_push_conflicts puts this rank's pushed arcs into the stable (qid, qs, input position)
 * order of their hits and counts consecutive ones whose hits had equal (qid,qs); if the sum over the ranks is > 0, mahip_sg_push_fix puts this rank's pushed arcs into the reference's hit order -- it
 * walks ALL hit keys, so the context must hold the whole input (mahip_set_full_input(c, 1), the default; a caller that only handed
 * over the rank's own records says 0 and gets an error here); (2) the ranks exchange their push-order rows
 * (mahip_asg_export_rows_push) and mahip_asg_import_push_rows builds the reference's arc order from the global push sequence. */
int mahip_set_full_input(mahip_ctx_t *c, int full);
int mahip_sg_push_conflicts(mahip_ctx_t *c, uint64_t *n_conf);
int mahip_sg_push_fix(mahip_ctx_t *c);
int mahip_asg_export_rows_push(mahip_ctx_t *c, void *d_dst);
int mahip_asg_import_push_rows(mahip_ctx_t *c, const void *d_src, const uint32_t *counts, int n_ranks, size_t stride);
/* asg.c:148-186 marking for the vertices [v_beg, v_end) only, no cleanup */
int mahip_asg_del_trans_range(mahip_ctx_t *c, int fuzz, uint32_t v_beg, uint32_t v_end, uint32_t *n_reduced);
/* the ol|del column of arcs [first, first+count) out of / into the graph */
int mahip_asg_flags_out(mahip_ctx_t *c, void *d_dst, size_t first, size_t count);
int mahip_asg_flags_in(mahip_ctx_t *c, const void *d_src, size_t first, size_t count);
/* asg.c:72-80 asg_cleanup on the current graph */
int mahip_asg_cleanup(mahip_ctx_t *c, uint32_t *n_arc);

/* ---- collectives of the sharded mode (csrc/comm.hip), queued on the context's stream ----------------------------------
 * RCCL (librccl opened at run time): rank 0 makes an id, everybody calls mahip_comm_init with it.  mahip_comm_init_shm is a
 * host-staged test double over POSIX shared memory for boxes with a single GPU (N processes on one device). */
int mahip_comm_unique_id(void *id128);
int mahip_comm_init(mahip_ctx_t *c, const void *id128, int rank, int world);
int mahip_comm_init_shm(mahip_ctx_t *c, const char *name, int rank, int world);
void mahip_comm_destroy(mahip_ctx_t *c);
int mahip_comm_rank(mahip_ctx_t *c);
int mahip_comm_world(mahip_ctx_t *c);
int mahip_comm_active(mahip_ctx_t *c);   /* more than one rank -- or one RCCL rank with MA_RCCL_ONE_RANK=1 (the collectives really run) */
int mahip_comm_all_gather(mahip_ctx_t *c, const void *d_send, void *d_recv, size_t bytes_per_rank);  /* d_recv: world x bytes, rank-major */
int mahip_comm_all_reduce_max_u8(mahip_ctx_t *c, void *d_buf, size_t n);                               /* OR of 0/1 flag bytes */
int mahip_comm_all_reduce_sum_u64(mahip_ctx_t *c, uint64_t *h_vals, size_t n);                         /* <= 32 host counters */
/* A transport of the caller's own instead of RCCL / the shared-memory double: five callbacks on HOST buffers (0 = ok); the library stages the device buffers
 * through the host around them.  all_gather: every rank's `bytes` from send into recv, rank-major; all_to_all_v: as mahip_comm_all_to_all_v below (bytes[i *
 * world + j] from rank i to rank j, pieces back to back).  tests/test_dist_gloo.py: host/sharded.c over torch.distributed's gloo backend on the CPU build. */
typedef struct {
	void *user;
	int (*all_gather)(void *user, const void *send, void *recv, size_t bytes);
	int (*all_reduce_max_u8)(void *user, void *buf, size_t n);
	int (*all_reduce_sum_u64)(void *user, uint64_t *vals, size_t n);
	int (*all_reduce_sum_u32)(void *user, void *buf, size_t n);
	int (*all_to_all_v)(void *user, const void *send, void *recv, const uint64_t *bytes);
} mahip_comm_ext_t;
int mahip_comm_init_ext(mahip_ctx_t *c, int rank, int world, const mahip_comm_ext_t *ext);
/* for the ranks' own text ranges (host/ingest_sharded.c): a device-side sum of u32 words, a personalised exchange (bytes[i * world + j] = what rank i sends
 * to rank j, pieces back to back in destination order on the way out and in source order on the way in), and an all-gather of a few host words */
int mahip_comm_all_reduce_sum_u32(mahip_ctx_t *c, void *d_buf, size_t n);
int mahip_comm_all_to_all_v(mahip_ctx_t *c, const void *d_send, void *d_recv, const uint64_t *bytes);
int mahip_comm_all_gather_u64(mahip_ctx_t *c, const uint64_t *h_vals, size_t n, uint64_t *h_out);
int mahip_comm_barrier(mahip_ctx_t *c);
int mahip_xbuf(mahip_ctx_t *c, int slot, size_t bytes, void **d_ptr);                                  /* exchange buffers (slot 0 / 1) */

/* ---- text of the record dumps (-p paf, -p sg, -p bed) and of the unitig GFA (-p ug) written on the device (csrc/text_dev.hpp over csrc/text_core.h) ---- */
/* A length per record, the device-wide scan, one byte string per record, in slabs of records; every slab's text goes to the host and to a sink.
 * Byte for byte what the host formatters (host/pipeline.c: print_hits, print_subs; host/unitig_gfa.c: ma_sg_print, ma_ug_print) and the reference write.
 * The unitig GFA (asm.c:77-116) is three blocks in one record space: units (per unitig its S line with the circularising links of a circular unitig, then one `a`
 * record per member), links (one L record per unitig arc), summary (one x record per unitig).  With sequences an S line is cut into a head record, chunk records of
 * seq_chunk bases each (no formatting: bytes of the unitig arena) and a tail record, so that no record is longer than a line and the slabs keep their size. */
#define MAHIP_TEXT_PAF 1
#define MAHIP_TEXT_SG  2
#define MAHIP_TEXT_BED 3
#define MAHIP_TEXT_UG  4
#define MAHIP_TEXT_ROAD_HOST   1   /* nothing was written: the caller formats on the host */
#define MAHIP_TEXT_ROAD_DEVICE 2
#define MAHIP_TEXT_OK        0
#define MAHIP_TEXT_SWITCHED_OFF 1  /* MA_TEXT_DEVICE is 0 or unset (the default is the host formatter: DESIGN section 7 has the measurement behind it) */
#define MAHIP_TEXT_NOMEM     2     /* a device or host buffer could not be had */
#define MAHIP_TEXT_NO_NAMES  3     /* mahip_text_names has not described the reads the records name */
#define MAHIP_TEXT_NO_UG     4     /* the context holds no unitigs (mahip_ug_gen has not run, or found none) */
#define MAHIP_TEXT_NO_SEQ    5     /* sequences were asked for, but this context holds no finished arena of these unitigs (mahip_useq_end(c, NULL)) */
#define MAHIP_TEXT_SEQ_NUL   6     /* a NUL byte in the arena: the reference's %s would end the S line there, which is not imitated */
#define MAHIP_TEXT_TOO_MANY  7     /* the record space of the unitig GFA does not fit 32 bits */
typedef struct {
	int kind, road, reason;
	uint64_t n_records;      /* hits, arcs or reads looked at; ug: records of its record space = unitigs + members + links + unitigs, and with sequences one more per unitig and chunk */
	uint64_t n_lines;        /* lines written (a bed dump skips reads); ug: the '\n' bytes of the text */
	uint64_t text_bytes;
	uint64_t n_slabs, slab_records;
	uint64_t max_name;       /* longest name of the dictionary, bytes */
	uint64_t n_slow_lines;   /* lines of waves whose 64 lines did not fit the LDS tile: written byte by byte straight to device memory (ug: RECORDS of such waves, chunks included) */
	double laps_ms[4];       /* names upload, export of the records, format (lengths + scan + write kernels), copy to the host + sink */
	uint64_t n_seq_bytes;    /* ug with sequences: bases copied into S lines */
	uint64_t seq_chunk;      /* ug: bases per chunk record (MA_TEXT_SEQ_CHUNK); 0 for the record dumps */
} mahip_text_info_t;
/* 0 = ok; anything else ends the dump and becomes its return value */
typedef int (*mahip_text_sink_t)(void *arg, const char *text, size_t n);
/* the dictionary the records' ids index: n_seq names back to back in blob, name i = blob[off[i] .. off[i + 1]); del (optional): one byte per read, non-zero =
 * the bed dump skips it.  Copied to the device; stays until the next call. */
int mahip_text_names(mahip_ctx_t *c, const char *blob, const uint64_t *off, uint32_t n_seq, const uint8_t *del);
/* The dump in two steps.  prepare: records exported on the device (hits in the order of a hit dump, arcs of the cleaned graph, both in the squeezed numbering when
 * a squeeze map is pending; kept intervals of slot 0), every line's length, every buffer.  It decides the road, all or nothing, before a byte is written:
 * returns 0 with info->road = DEVICE, or 0 with road = HOST and a reason (nothing happened; the caller formats on the host), or -1 (error).
 * emit: the slabs' bytes to the sink.  The context must not be used for anything else in between.  dump = prepare + emit. */
int mahip_text_prepare(mahip_ctx_t *c, int kind, int have_sub, mahip_text_info_t *info);
int mahip_text_emit(mahip_ctx_t *c, mahip_text_sink_t sink, void *arg, mahip_text_info_t *info);
int mahip_text_dump(mahip_ctx_t *c, int kind, int have_sub, mahip_text_sink_t sink, void *arg, mahip_text_info_t *info);
int mahip_text_last(mahip_ctx_t *c, mahip_text_info_t *info);
/* prepare for the unitig GFA: works from the unitigs mahip_ug_gen left in the context (the members never come down), the names of mahip_text_names and the kept
 * intervals of slot 0 (squeezed as for the sg kind).  links: the unitig arcs in the reference's order -- mahip_ug_download(c, 0, 0, 0, 0, 0, 0, arcs) then
 * ma_refsort_arcs, as asg_cleanup leaves them (equal keys included, that order stays the host's); the per-end arc counts of the x lines are counted from them.
 * with_seq: the S lines carry the unitigs' bases, taken from the arena mahip_useq_end(c, NULL) left in THIS context (anything else: road HOST, reason NO_SEQ).
 * Where every unitig's bases start in it (asm.c:250) is the uoff of mahip_useq_plan when the context holds a plan of these unitigs; otherwise the lengths come down,
 * are summed up on the host and the offsets go up.  The same all-or-nothing decision as mahip_text_prepare, followed by the same mahip_text_emit. */
int mahip_text_prepare_ug(mahip_ctx_t *c, int have_sub, const asg_arc_t *links, uint32_t n_links, int with_seq, mahip_text_info_t *info);
/* stage entry (tests): hand-made records (ma_hit_t / asg_arc_t; none for bed, where n_records = n_seq), kept intervals (ma_sub_t, n_seq of them, or 0), del flags and
 * names from host memory, formatted on the device whatever MA_TEXT_DEVICE says, in slabs of `slab` records (0: the default); *text is malloc'ed */
int mahip_text_format_mem(mahip_ctx_t *c, int kind, const void *records, uint64_t n_records, const void *sub, uint32_t n_seq, const uint8_t *del,
                          const char *blob, const uint64_t *off, uint64_t slab, char **text, size_t *len, mahip_text_info_t *info);
/* stage entry (tests) for the unitig GFA: n_utg hand-made unitigs (u_n members each, back to back in `members`; u_start == 0xffffffff: circular), link records in
 * output order, counts[2 i + e] = arcs leaving end e of unitig i, kept intervals (or 0); with_seq != 0: the S lines carry bases from `arena`, an image laid out as
 * ma_ug_seq lays it out (unitig strings back to back, one spare byte behind each; arena == 0: refused with NO_SEQ).  Formats on the device whatever MA_TEXT_DEVICE
 * says.  A refusal returns 0 with info->road = HOST, a reason and *text = NULL. */
int mahip_text_format_ug_mem(mahip_ctx_t *c, uint32_t n_utg, const uint32_t *u_n, const uint32_t *u_len, const uint32_t *u_start, const uint32_t *u_end, const uint64_t *members,
                             const asg_arc_t *links, uint32_t n_links, const uint32_t *counts, const void *sub, uint32_t n_seq, int with_seq, const char *arena, uint64_t arena_bytes,
                             const char *blob, const uint64_t *off, uint64_t slab, char **text, size_t *len, mahip_text_info_t *info);
/* MA_TEXT_DEVICE: 1 on, 0 off; unset: off (the device road wins by far where the text is gigabytes, stays inside the noise where it is megabytes) */
int mahip_text_enabled(void);

/* ---- instrumentation -------------------------------------------------------------------------------- */
/* Per-kernel timing with HIP events on the launch stream.  enable=1 brackets every kernel launch with
 * events (adds launch overhead; use for measurement runs only). */
int mahip_prof_enable(mahip_ctx_t *c, int enable);
int mahip_prof_reset(mahip_ctx_t *c);
/* writes up to max entries; returns the number of distinct kernels seen */
typedef struct { const char *name; uint64_t launches; double total_ms; double alg_bytes; } mahip_prof_t;
int mahip_prof_get(mahip_ctx_t *c, mahip_prof_t *out, int max);
/* phase marks: an event on the stream per slot (0..63); after a sync, ms[i] = time from mark first+i to mark first+i+1 (0 if either is missing) */
int mahip_mark(mahip_ctx_t *c, int slot);
int mahip_marks_ms(mahip_ctx_t *c, int first, int n, float *ms);
/* bytes of HBM currently held by the context: buffers in use + what its pool keeps idle for the next request */
size_t mahip_mem_bytes(mahip_ctx_t *c);
/* the idle part alone, and a way to hand it back to the driver (whole free allocations; waits for the context's stream).  A context whose
 * allocation fails trims itself and the process's other contexts on the same GPU on its own; other PROCESSES that share the GPU
 * (MA_COMM=shm ranks) are what this call is for: the sharded head calls it at its end.  released (optional) = bytes returned. */
size_t mahip_mem_pool_bytes(mahip_ctx_t *c);
int mahip_mem_trim(mahip_ctx_t *c, size_t *released);

/* Measurement hooks (csrc/diag.hip; tools/pmc_calibrate.py) -- NOT part of the pipeline: plain access patterns with a known byte count (a 16-byte
 * stream, 8 bytes of every 32-byte record, a random 32-byte fetch, the run-wise scatter of a radix pass, ...), timed with HIP events on the context's
 * stream.  They give the rate this GPU sustains for the patterns the hot path is made of, and a known byte count per pattern to calibrate rocprofv3's
 * FETCH_SIZE / WRITE_SIZE against.  mahip_diag_run: `reps` launches of `pattern` over `bytes` of data; *best_ms = the fastest, *moved = bytes read +
 * written by construction.  0 on success. */
int mahip_diag_patterns(void);
const char *mahip_diag_name(int pattern);
int mahip_diag_run(mahip_ctx_t *c, int pattern, size_t bytes, int reps, double *best_ms, double *moved);
/* device pointers for multi-GPU exchanges done outside (RCCL via torch.distributed): which = MAHIP_PTR_* */
#define MAHIP_PTR_SUB0    0
#define MAHIP_PTR_SUB1    1
#define MAHIP_PTR_RDFLAG  2
void *mahip_devptr(mahip_ctx_t *c, int which, size_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
