/* ingest_gpu.c -- the text part of ma_hit_read (reference hit.c:70-101, paf.c, sdict.c) on the device.
 *
 * The host only moves bytes: a plain file goes from the page cache straight into pinned staging slots and on to
 * HBM (mahip_paf_load_fd); a bgzip-compressed (BGZF) file goes to HBM as it is and is inflated there, one wave per block (mahip_bgzf_load_fd; the walk over
 * its member chain is below); a plain gzip file, one member or several, can be cut into chunks and inflated there too (MA_GZIP_DEVICE=1: mahip_gzip_load_fd_members; headers and trailers are
 * read below); otherwise gzip / stdin input is read by zlib (as the reference does through gzread) one PIECE of whole lines at a time, and piece k is uploaded
 * and parsed (mahip_paf_stream_piece_mem) while a second thread inflates piece k + 1 (ma_hit_ingest_stream below); MA_INGEST_STREAM=0, -R (unless
 * MA_STREAM_NOCONT=1: ma_hit_ingest_stream_excl) and ma_paf_load_file inflate the whole text into memory first and upload it.  Lines, columns, numbers, the span/match filter, the name dictionary with the reference's
 * first-appearance ids and the (mirrored) hit records are all produced by csrc/paf.hip; what comes back is the
 * dictionary (names + first-seen lengths, R entries) and, only for the per-symbol ABI, the records.
 * The -R pre-filter (ma_hit_no_cont, hit.c:38-68) rides in the same parse: the exclusion is a flag per name.
 * MA_HOST_PARSE=1 forces the host reader (ingest_mt.c / paf_reader.c); both are pinned to the same records and ids.
 */
#define _GNU_SOURCE /* memrchr */
#include <fcntl.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include "ma_host.h"

#define GPU(call) do { if ((call) != 0) ma_gpu_fail(__func__); } while (0)
/* the text stage may simply not fit (text + 61 B of columns per line + the records): report -2 and let the caller fall
 * back to the host reader, which streams the file and only needs the records on the device */
#define GPU_SOFT(call) do { if ((call) != 0) { fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; } } while (0)

static char *slurp_gz(gzFile fp, size_t *len)
{
	size_t n = 0, m = 64u << 20;
	char *buf = (char*)malloc(m);
	for (;;) {
		int got;
		if (m - n < (16u << 20)) { m += m >> 1; buf = (char*)realloc(buf, m); }
		got = gzread(fp, buf + n, (unsigned)((m - n) < (1u << 30) ? (m - n) : (1u << 30)));
		if (got <= 0) break;
		n += (size_t)got;
	}
	*len = n;
	return buf;
}

/* ---- BGZF: the member chain of a bgzip-compressed file -> the block table of include/mahip.h (RFC 1952 + the BGZF convention of the SAM specification).
 * The walk is a dependent chain: a member's size stands in its own header.  One read of BG_READ bytes at a member's last 8 bytes yields its trailer (CRC32,
 * ISIZE) AND the next member's header, so the chain costs one small read per member.  src: an open regular file (fd >= 0) or an image in memory. */
#define BG_READ 96
typedef struct { int fd; const unsigned char *mem; uint64_t n, woff, wlen; unsigned char w[BG_READ]; } bg_src_t;
/* bytes [off, off + len) of the source, len <= BG_READ, off + len <= n; 0 ok, -1 read error */
static int bg_get(bg_src_t *s, uint64_t off, unsigned len, unsigned char *out)
{
	if (s->mem) { memcpy(out, s->mem + off, len); return 0; }
	if (off < s->woff || off + len > s->woff + s->wlen) {
		uint64_t want = s->n - off < BG_READ ? s->n - off : BG_READ, got = 0;
		while (got < want) {
			ssize_t r = pread(s->fd, s->w + got, (size_t)(want - got), (off_t)(off + got));
			if (r <= 0) return -1;
			got += (uint64_t)r;
		}
		s->woff = off; s->wlen = want;
	}
	memcpy(out, s->w + (off - s->woff), len);
	return 0;
}
static uint32_t bg_le32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* returns a MAHIP_BGZF_* reason (MAHIP_BGZF_OK: *tab holds *n_members rows, malloc'ed; otherwise *bad = the member the walk stopped at and *tab = 0), -1 on a
 * read error.  out_off is the 64-bit exclusive prefix sum of ISIZE. */
int ma_bgzf_walk(int fd, const void *mem, uint64_t nbytes, mahip_bgzf_member_t **tab, uint64_t *n_members, uint64_t *n_empty, uint64_t *text_bytes, int64_t *bad)
{
	bg_src_t src;
	mahip_bgzf_member_t *t = 0;
	uint64_t n = 0, m = 0, p = 0, text = 0, empty = 0;
	int reason = MAHIP_BGZF_OK;
	memset(&src, 0, sizeof(src));
	src.fd = fd; src.mem = (const unsigned char*)mem; src.n = nbytes;
	*tab = 0; *n_members = *n_empty = *text_bytes = 0; *bad = -1;
	while (p < nbytes) {
		unsigned char h[12], sf[4], tr[8];
		uint64_t total = 0, x, xend;
		uint32_t xlen, isize;
		int have_bc = 0;
#define BG_STOP(r) { reason = (r); break; }
		if (nbytes - p < 12) BG_STOP(n ? MAHIP_BGZF_TRAILING : MAHIP_BGZF_NOT_BGZF)
		if (bg_get(&src, p, 12, h) != 0) { free(t); return -1; }
		if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) BG_STOP(n ? MAHIP_BGZF_TRAILING : MAHIP_BGZF_NOT_BGZF)
		if (!(h[3] & 4)) BG_STOP(n ? MAHIP_BGZF_NO_BC : MAHIP_BGZF_NOT_BGZF) /* no extra field */
		if (h[3] & ~(4 | 1)) BG_STOP(MAHIP_BGZF_BAD_FLG)                      /* FTEXT adds no field; FHCRC, FNAME, FCOMMENT and the reserved bits are not handled */
		xlen = (uint32_t)h[10] | (uint32_t)h[11] << 8;
		x = p + 12; xend = x + xlen;
		if (xend > nbytes) BG_STOP(MAHIP_BGZF_PAST_END)
		while (xend - x >= 4) { /* subfields SI1 SI2 SLEN data; `BC` may stand behind others */
			uint32_t slen;
			if (bg_get(&src, x, 4, sf) != 0) { free(t); return -1; }
			slen = (uint32_t)sf[2] | (uint32_t)sf[3] << 8;
			if (xend - x - 4 < slen) break; /* a subfield that runs out of the extra field */
			if (sf[0] == 'B' && sf[1] == 'C' && slen == 2) {
				unsigned char bs[2];
				if (bg_get(&src, x + 4, 2, bs) != 0) { free(t); return -1; }
				total = ((uint64_t)bs[0] | (uint64_t)bs[1] << 8) + 1; /* BSIZE + 1: the whole member */
				have_bc = 1;
				break;
			}
			x += 4 + slen;
		}
		if (!have_bc) BG_STOP(n ? MAHIP_BGZF_NO_BC : MAHIP_BGZF_NOT_BGZF)
		if (total > nbytes - p || total < 12 + (uint64_t)xlen + 8) BG_STOP(MAHIP_BGZF_PAST_END)
		if (bg_get(&src, p + total - 8, 8, tr) != 0) { free(t); return -1; }
		isize = bg_le32(tr + 4);
		if (isize > 65536) BG_STOP(MAHIP_BGZF_ISIZE)
#undef BG_STOP
		if (n == m) {
			mahip_bgzf_member_t *t2;
			m = m ? m + (m >> 1) : (nbytes >> 14) + 16; /* bgzip's members hold 64 KiB of text: a quarter of that compressed is a fair first guess */
			t2 = (mahip_bgzf_member_t*)realloc(t, (size_t)m * sizeof(*t));
			if (t2 == 0) { free(t); return -1; }
			t = t2;
		}
		t[n].in_off = xend; t[n].in_len = (uint32_t)(total - 12 - xlen - 8);
		t[n].out_off = text; t[n].isize = isize; t[n].crc = bg_le32(tr); t[n].pad = 0;
		text += isize; empty += isize == 0;
		++n; p += total;
	}
	if (reason == MAHIP_BGZF_OK && n == 0) reason = MAHIP_BGZF_NOT_BGZF; /* an empty source */
	if (reason != MAHIP_BGZF_OK) { *bad = (int64_t)n; free(t); return reason; }
	*tab = t; *n_members = n; *n_empty = empty; *text_bytes = text;
	return MAHIP_BGZF_OK;
}

/* ---- plain gzip: a member's header and trailer (RFC 1952) at any offset of the file; which offsets begin a member the device finds out (include/mahip.h).
 * ma_gzip_head_at: the header at byte `off`: MAHIP_GZIP_OK (*hdr_len = its length: the deflate stream starts at off + *hdr_len, and at least a trailer's 8 bytes
 * follow) or MAHIP_GZIP_BAD_HEADER; -1 on a read error */
int ma_gzip_head_at(int fd, const void *mem, uint64_t nbytes, uint64_t off, uint64_t *hdr_len)
{
	bg_src_t src;
	unsigned char h[12], b[8];
	uint64_t p = off + 10;
	int k;
	memset(&src, 0, sizeof(src));
	src.fd = fd; src.mem = (const unsigned char*)mem; src.n = nbytes;
	*hdr_len = 0;
	if (off > nbytes || nbytes - off < 10 + 8) return MAHIP_GZIP_BAD_HEADER;
	if (bg_get(&src, off, 10, h) != 0) return -1;
	if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe0)) return MAHIP_GZIP_BAD_HEADER; /* CM 8; FLG bits 5..7 are reserved */
	if (h[3] & 4) { /* FEXTRA: skipped, unless a `BC` subfield says that this is BGZF's business */
		uint64_t x, xend;
		if (nbytes - p < 2) return MAHIP_GZIP_BAD_HEADER;
		if (bg_get(&src, p, 2, b) != 0) return -1;
		x = p + 2; xend = x + ((uint64_t)b[0] | (uint64_t)b[1] << 8);
		if (xend > nbytes) return MAHIP_GZIP_BAD_HEADER;
		while (xend - x >= 4) {
			uint32_t slen;
			if (bg_get(&src, x, 4, b) != 0) return -1;
			slen = (uint32_t)b[2] | (uint32_t)b[3] << 8;
			if (xend - x - 4 < slen) break;
			if (b[0] == 'B' && b[1] == 'C' && slen == 2) return MAHIP_GZIP_BAD_HEADER;
			x += 4 + slen;
		}
		p = xend;
	}
	for (k = 0; k < 2; ++k) /* FNAME, FCOMMENT: zero-terminated */
		if (h[3] & (k == 0 ? 8 : 16)) {
			for (;;) {
				if (p >= nbytes) return MAHIP_GZIP_BAD_HEADER;
				if (bg_get(&src, p, 1, b) != 0) return -1;
				++p;
				if (b[0] == 0) break;
			}
		}
	if (h[3] & 2) p += 2; /* FHCRC */
	if (p > nbytes || nbytes - p < 8) return MAHIP_GZIP_BAD_HEADER;
	*hdr_len = p - off;
	return MAHIP_GZIP_OK;
}

/* the trailer whose 8 bytes start at byte `off`: 0, or -1 on a read error (or when it does not lie in the file) */
int ma_gzip_trailer_at(int fd, const void *mem, uint64_t nbytes, uint64_t off, uint32_t *crc, uint32_t *isize)
{
	bg_src_t src;
	unsigned char b[8];
	memset(&src, 0, sizeof(src));
	src.fd = fd; src.mem = (const unsigned char*)mem; src.n = nbytes;
	*crc = *isize = 0;
	if (off > nbytes || nbytes - off < 8 || bg_get(&src, off, 8, b) != 0) return -1;
	*crc = bg_le32(b); *isize = bg_le32(b + 4);
	return 0;
}

/* MA_GZIP_CAND_CAP: the capacity of the member scan's candidate list (tests make it small); anything else is the default */
size_t ma_gzip_cand_cap(void)
{
	const char *s = getenv("MA_GZIP_CAND_CAP");
	long long v = s ? atoll(s) : 0;
	if (v >= 1 && v <= (1ll << 24)) return (size_t)v;
	return MAHIP_GZIP_CAND_CAP_DEFAULT;
}

/* MA_GZIP_CHUNK: bytes of payload per chunk, a power of two in 1024 .. 16 MiB; anything else is the default */
size_t ma_gzip_chunk(void)
{
	const char *s = getenv("MA_GZIP_CHUNK");
	long long v = s ? atoll(s) : 0;
	if (v >= 1024 && v <= (16ll << 20) && (v & (v - 1)) == 0) return (size_t)v;
	return MAHIP_GZIP_CHUNK_DEFAULT;
}

/* MA_GZIP_DEVICE=0|1: plain gzip files on the device road; unset: MA_GZIP_DEVICE_DEFAULT (DESIGN 7 has the measurement it follows from) */
#define MA_GZIP_DEVICE_DEFAULT 0
int ma_gzip_device_enabled(void)
{
	const char *s = getenv("MA_GZIP_DEVICE");
	return s && *s ? atoi(s) != 0 : MA_GZIP_DEVICE_DEFAULT;
}

int ma_bgzf_enabled(void)
{
	const char *s = getenv("MA_BGZF_HOST");
	return !(s && atoi(s) != 0);
}

int ma_gpu_parse_enabled(void)
{
	const char *s = getenv("MA_HOST_PARSE");
	return !(s && atoi(s) != 0);
}

static void ingest_dictionary(mahip_ctx_t *c, const mahip_paf_info_t *pi, sdict_t *d, size_t *n_hits, int release, double t1);

/* parse the text already loaded into the context (mahip_paf_load_*): records stay on the device, the dictionary is
 * rebuilt in d (which must be empty or a previous result of this function); release = free the text afterwards */
int ma_hit_ingest_loaded(mahip_ctx_t *c, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int release)
{
	return ma_hit_ingest_loaded_excl(c, min_span, min_match, d, n_hits, bi_dir, release, 0, 0, 0.f);
}

/* no_cont: -R, the reference's Step 0 (hit.c:38-68) folded into the same parse; prints its log line first */
int ma_hit_ingest_loaded_excl(mahip_ctx_t *c, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int release, int no_cont, int max_hang, float int_frac)
{
	double t1 = sys_realtime();
	mahip_paf_info_t info;
	GPU(mahip_set_shard(c, 0, 0xffffffffu));
	GPU_SOFT(mahip_paf_parse_excl(c, min_span, min_match, bi_dir, no_cont, max_hang, int_frac, &info));
	if (no_cont) {
		if (ma_verbose >= 3) fprintf(MA_LOG, "[M::%s::%s] dropped %d contained reads\n", "ma_hit_no_cont", sys_timestamp(), info.n_excl);
		fprintf(MA_LOG, "[M::%s] ===> Step 1: reading read mappings <===\n", "main");
	}
	ingest_dictionary(c, &info, d, n_hits, release, t1);
	return 0;
}

/* what follows a parse, whole or streamed: the dictionary comes to the host, the reference's log line (hit.c:102) */
static void ingest_dictionary(mahip_ctx_t *c, const mahip_paf_info_t *pi, sdict_t *d, size_t *n_hits, int release, double t1)
{
	const int timing = ma_timing_level() >= 1;
	const mahip_paf_info_t info = *pi;
	double t2 = sys_realtime(), t3;
	size_t tot_len = 0;
	/* the dictionary: the names in one block (the dictionary's arena) and the sd_seq_t records the device wrote for that block -- two copies, no
	 * per-name work on the host */
	{
		char *names = 0;
		sd_seq_t *seq = 0;
		uint64_t tl = 0;
		if (!ma_sd_recycle(d, info.name_bytes, info.n_seq, &names, &seq)) { /* (the same dictionary filled again keeps its blocks) */
			names = (char*)ma_big_alloc(info.name_bytes ? info.name_bytes : 1);
			seq = (sd_seq_t*)ma_big_alloc(((size_t)info.n_seq + 1) * sizeof(sd_seq_t));
		}
		GPU(mahip_paf_seqs(c, names, seq, &tl));
		ma_sd_adopt(d, names, info.name_bytes, info.n_seq, seq);
		tot_len = (size_t)tl;
	}
	if (release) GPU(mahip_paf_release(c));
	t3 = sys_realtime();
	if (ma_verbose >= 3)
		fprintf(MA_LOG, "[M::%s::%s] read %ld hits; stored %ld hits and %d sequences (%ld bp)\n", "ma_hit_read", sys_timestamp(), (long)info.n_records, (long)info.n_hits, d->n_seq, (long)tot_len);
	if (timing) fprintf(stderr, "[T::ingest_gpu] parse %.3f  dictionary%s %.3f s (%lu lines)\n", t2 - t1, release ? "+release" : "", t3 - t2, (unsigned long)info.n_lines);
	*n_hits = (size_t)info.n_hits;
}

/* file -> HBM; 0 ok, -1 = could not open, -2 = the device refused.  The ladder: a plain file whole, bgzip on the device, plain gzip on the device when enabled, and
 * on the last rung zlib on the host.  stream_fp == 0: the last rung inflates everything and uploads it.  Otherwise the last rung is left to the caller: 1 is
 * returned with the input open in *stream_fp (*seekable: a regular file, which a reader that starts over can open again); force_stream: every input goes that way. */
static int paf_load_ladder(mahip_ctx_t *c, const char *fn, gzFile *stream_fp, int *seekable, int force_stream)
{
	int fd = -1, is_plain = 0, is_reg = 0;
	struct stat st;
	if (seekable) *seekable = 0;
	if (fn && strcmp(fn, "-") != 0) {
		unsigned char magic[2] = { 0, 0 };
		fd = open(fn, O_RDONLY);
		if (fd < 0) return -1;
		if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
			ssize_t r = pread(fd, magic, 2, 0);
			is_reg = 1;
			is_plain = !(r == 2 && magic[0] == 0x1f && magic[1] == 0x8b);
		}
	}
	if (seekable) *seekable = is_reg;
	if (stream_fp && force_stream) {
		*stream_fp = fd >= 0 ? gzdopen(fd, "r") : gzdopen(fileno(stdin), "r");
		if (*stream_fp == 0) { if (fd >= 0) close(fd); return -1; }
		return 1;
	}
	if (is_plain) {
		if (mahip_paf_load_fd(c, fd, (size_t)st.st_size) != 0) { close(fd); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
		close(fd);
	} else {
		gzFile fp;
		if (is_reg) { /* bgzip's blocks are inflated on the device (include/mahip.h); whatever keeps it from that leaves the file to zlib, as before */
			mahip_bgzf_info_t bi;
			if (!ma_bgzf_enabled()) {
				memset(&bi, 0, sizeof(bi));
				bi.reader = MAHIP_BGZF_HOST; bi.reason = MAHIP_BGZF_FORCED; bi.first_bad_member = -1; bi.comp_bytes = (uint64_t)st.st_size;
				mahip_bgzf_note(c, &bi);
			} else {
				if (mahip_bgzf_load_fd(c, fd, (size_t)st.st_size, MAHIP_BGZF_PAF, &bi) != 0) { close(fd); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
				if (bi.reason == MAHIP_BGZF_OK) { close(fd); return 0; }
				if (bi.reason == MAHIP_BGZF_NOT_BGZF) { /* plain gzip: deflate streams (one a member; `cat a.gz b.gz` has several), cut into chunks on the device (include/mahip.h); any reason leaves it to zlib */
					mahip_gzip_info_t gi;
					if (!ma_gzip_device_enabled()) {
						memset(&gi, 0, sizeof(gi));
						gi.reader = MAHIP_BGZF_HOST; gi.reason = MAHIP_GZIP_FORCED; gi.first_bad_item = -1; gi.comp_bytes = (uint64_t)st.st_size;
						mahip_gzip_note(c, &gi);
						if (ma_timing_level() >= 1) fprintf(stderr, "[T::gzip] reader=host reason=%d (%s) item=-1 chunks=0 items=0\n", gi.reason, mahip_gzip_reason_name(gi.reason));
					} else {
						if (mahip_gzip_load_fd_members(c, fd, (size_t)st.st_size, MAHIP_BGZF_PAF, 0, &gi) != 0) { close(fd); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
						if (gi.reason == MAHIP_GZIP_OK) { close(fd); return 0; }
					}
				}
			}
		}
		fp = fd >= 0 ? gzdopen(fd, "r") : gzdopen(fileno(stdin), "r");
		size_t len = 0;
		char *buf;
		if (fp == 0) { if (fd >= 0) close(fd); return -1; }
		if (stream_fp) { *stream_fp = fp; return 1; }
		gzbuffer(fp, 1u << 20);
		buf = slurp_gz(fp, &len);
		gzclose(fp);
		if (mahip_paf_load_mem(c, buf, len) != 0) { free(buf); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
		free(buf);
	}
	return 0;
}

int ma_paf_load_file(mahip_ctx_t *c, const char *fn) { return paf_load_ladder(c, fn, 0, 0, 0); }

/* MA_INGEST_STREAM: 0 = gzip / stdin input is inflated whole before the first byte is uploaded; 1 = EVERY input is streamed piece by piece, plain, bgzip and gzip
 * files too (tests reach the streamed road with any file); unset: MA_INGEST_STREAM_DEFAULT, where -1 = stream what reaches the ladder's last rung (DESIGN 7 has
 * the measurement the default follows from) */
#define MA_INGEST_STREAM_DEFAULT -1
int ma_ingest_stream_mode(void)
{
	const char *s = getenv("MA_INGEST_STREAM");
	return s && *s ? (atoi(s) != 0) : MA_INGEST_STREAM_DEFAULT;
}
/* MA_STREAM_NOCONT: 1 = with -R, too, what reaches the ladder's last rung is streamed; off by default */
int ma_stream_nocont(void)
{
	const char *s = getenv("MA_STREAM_NOCONT");
	return s && *s && atoi(s) != 0;
}
/* MA_INGEST_PIECE: bytes of text per piece, clamped to [256, 1 GiB] */
#define MA_INGEST_PIECE_DEFAULT ((size_t)16 << 20)
size_t ma_ingest_piece(void)
{
	const char *s = getenv("MA_INGEST_PIECE");
	long long v = s && *s ? atoll(s) : (long long)MA_INGEST_PIECE_DEFAULT;
	return v < 256 ? (size_t)256 : v > (1ll << 30) ? (size_t)1 << 30 : (size_t)v;
}

/* ---- cut and carry.  The reader hands out pieces of WHOLE LINES: it fills a buffer with what the last piece left over (the carry: the bytes behind its last
 * newline) and `piece` more bytes, cuts behind the last newline (memrchr) and keeps the rest for the next piece.  A buffer without any newline grows by another
 * `piece` and is read on, so a line longer than a piece -- than any number of pieces -- is one piece.  The end of the input hands over what is left, newline or
 * not, as the last piece.  The source is a callback, so that tests/stream_cut_main.c can drive the same code from a pipe with small buffers. */
int ma_cut_next(ma_cut_t *k, char **buf, size_t *cap, size_t *len, int *last)
{
	size_t n = k->carry_len, target;
	if (*cap < n + k->piece) {
		char *nb = (char*)realloc(*buf, n + k->piece);
		if (nb == 0) return -1;
		*buf = nb; *cap = n + k->piece;
	}
	if (n) memcpy(*buf, k->carry, n);
	k->carry_len = 0;
	target = n + k->piece;
	for (;;) {
		while (n < target) {
			size_t want = target - n < ((size_t)1 << 30) ? target - n : (size_t)1 << 30;
			long got = k->read(k->src, *buf + n, want);
			if (got <= 0) { *len = n; *last = 1; return 0; } /* the end (zlib reports a damaged stream the same way; what it gave so far counts, as in the reference) */
			n += (size_t)got;
		}
		{
			const char *nl = (const char*)memrchr(*buf, '\n', n);
			if (nl) {
				const size_t cut = (size_t)(nl - *buf) + 1, rest = n - cut;
				if (rest > k->carry_cap) {
					char *nc = (char*)realloc(k->carry, rest);
					if (nc == 0) return -1;
					k->carry = nc; k->carry_cap = rest;
				}
				if (rest) memcpy(k->carry, *buf + cut, rest);
				k->carry_len = rest;
				*len = cut; *last = 0;
				return 0;
			}
		}
		{ /* one line so far: more room, read on */
			char *nb = (char*)realloc(*buf, *cap + k->piece);
			if (nb == 0) return -1;
			*buf = nb; *cap += k->piece; target += k->piece;
		}
	}
}

static long gz_read_cb(void *src, char *dst, size_t want) { return (long)gzread((gzFile)src, dst, (unsigned)want); }

/* two buffers between the producer (zlib + the cut) and the calling thread (upload + the device's work on the piece): ma_stream_q_t of ma_host.h; the streamed
 * PAF ingest below and the streamed reads-file reader (unitig_gfa.c) share it */
static void *stream_producer(void *arg)
{
	ma_stream_q_t *q = (ma_stream_q_t*)arg;
	int i = 0;
	for (;; i ^= 1) {
		double t0;
		int rc;
		pthread_mutex_lock(&q->mu);
		while (q->b[i].full && !q->stop) pthread_cond_wait(&q->cv, &q->mu);
		if (q->stop) { pthread_mutex_unlock(&q->mu); break; }
		pthread_mutex_unlock(&q->mu);
		t0 = sys_realtime();
		rc = ma_cut_next(&q->cut, &q->b[i].p, &q->b[i].cap, &q->b[i].len, &q->b[i].last);
		q->t_prod += sys_realtime() - t0;
		pthread_mutex_lock(&q->mu);
		if (rc != 0) { q->failed = 1; q->b[i].len = 0; q->b[i].last = 1; }
		q->b[i].full = 1;
		pthread_cond_broadcast(&q->cv);
		pthread_mutex_unlock(&q->mu);
		if (q->b[i].last) break;
	}
	return 0;
}

void ma_stream_q_init(ma_stream_q_t *q, gzFile fp, size_t piece_bytes)
{
	memset(q, 0, sizeof(*q));
	q->cut.piece = piece_bytes; q->cut.read = gz_read_cb; q->cut.src = fp;
	gzbuffer(fp, 1u << 20);
	pthread_mutex_init(&q->mu, 0);
	pthread_cond_init(&q->cv, 0);
}
int ma_stream_q_start(ma_stream_q_t *q) { q->started = pthread_create(&q->th, 0, stream_producer, q) == 0; return q->started ? 0 : -1; }
/* buffer i holds the next piece when this returns (the time waited goes to q->t_wait); -1: the producer ran out of memory */
int ma_stream_q_wait(ma_stream_q_t *q, int i)
{
	const double w0 = sys_realtime();
	pthread_mutex_lock(&q->mu);
	while (!q->b[i].full) pthread_cond_wait(&q->cv, &q->mu);
	pthread_mutex_unlock(&q->mu);
	q->t_wait += sys_realtime() - w0;
	return q->failed ? -1 : 0;
}
/* buffer i goes back to the producer; stop: the consumer gives up -- the producer finishes the piece it is at and ends */
void ma_stream_q_release(ma_stream_q_t *q, int i, int stop)
{
	pthread_mutex_lock(&q->mu);
	q->b[i].full = 0;
	if (stop) q->stop = 1;
	pthread_cond_broadcast(&q->cv);
	pthread_mutex_unlock(&q->mu);
}
/* the consumer gives up but KEEPS every buffer as it is: the producer finishes the piece it is at and ends; afterwards b[] and cut.carry hold what was read ahead */
void ma_stream_q_halt(ma_stream_q_t *q)
{
	pthread_mutex_lock(&q->mu);
	q->stop = 1;
	pthread_cond_broadcast(&q->cv);
	pthread_mutex_unlock(&q->mu);
	ma_stream_q_join(q);
}
void ma_stream_q_join(ma_stream_q_t *q) { if (q->started) { pthread_join(q->th, 0); q->started = 0; } }
void ma_stream_q_destroy(ma_stream_q_t *q)
{
	ma_stream_q_join(q);
	free(q->b[0].p); free(q->b[1].p); free(q->cut.carry);
	pthread_mutex_destroy(&q->mu);
	pthread_cond_destroy(&q->cv);
}

/* the text behind fp (plain or gzip, file or pipe) piece by piece through the streamed parse: 0 = the records are in the context and d holds the dictionary, as
 * after ma_hit_ingest_loaded; -2 = the device refused (the stream is aborted, the text stage released; fp has been read from).  fp stays open. */
int ma_hit_ingest_stream(mahip_ctx_t *c, gzFile fp, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, size_t piece_bytes)
{
	return ma_hit_ingest_stream_excl(c, fp, min_span, min_match, d, n_hits, bi_dir, piece_bytes, 0, 0, 0.f);
}

/* no_cont: -R in the same single pass (mahip_paf_stream_begin_excl: provisional ids, renumbered at the end); prints the reference's log lines of Step 0 first,
 * as ma_hit_ingest_loaded_excl does */
int ma_hit_ingest_stream_excl(mahip_ctx_t *c, gzFile fp, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, size_t piece_bytes, int no_cont, int max_hang, float int_frac)
{
	const int timing = ma_timing_level() >= 1;
	const double t0 = sys_realtime();
	ma_stream_q_t q;
	mahip_paf_info_t info;
	mahip_paf_stream_report_t sr;
	mahip_paf_stream_excl_report_t xr;
	int i = 0, bad = 0;
	memset(&sr, 0, sizeof(sr));
	memset(&xr, 0, sizeof(xr));
	ma_stream_q_init(&q, fp, piece_bytes);
	GPU(mahip_set_shard(c, 0, 0xffffffffu));
	if (mahip_paf_stream_begin_excl(c, min_span, min_match, bi_dir, no_cont, max_hang, int_frac) != 0) bad = 1;
	if (!bad && ma_stream_q_start(&q) != 0) { mahip_paf_stream_abort(c); ma_gpu_fail(__func__); }
	for (; !bad; i ^= 1) {
		int last;
		if (ma_stream_q_wait(&q, i) != 0) { fprintf(stderr, "[E::%s] out of memory for a piece of the input\n", __func__); exit(1); }
		last = q.b[i].last;
		if (mahip_paf_stream_piece_mem(c, q.b[i].p, q.b[i].len, last) != 0) bad = 1;
		ma_stream_q_release(&q, i, bad);
		if (last || bad) { ma_stream_q_join(&q); break; }
	}
	if (!bad && mahip_paf_stream_end(c, &info) != 0) bad = 1;
	mahip_paf_stream_last(c, &sr);
	mahip_paf_stream_excl_last(c, &xr);
	ma_stream_q_destroy(&q);
	if (bad) {
		fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror());
		mahip_paf_stream_abort(c);
		mahip_paf_release(c);
		return -2;
	}
	if (timing)
		fprintf(stderr, "[T::ingest_gpu] stream: pieces=%lu piece=%lu B producer %.3f upload %.3f parse %.3f fold %.3f waited-for-input %.3f s\n", (unsigned long)sr.n_pieces,
		        (unsigned long)piece_bytes, q.t_prod, sr.t_upload, sr.t_parse, sr.t_fold, q.t_wait);
	if (timing && no_cont)
		fprintf(stderr, "[T::ingest_gpu] stream: -R dropped early %lu lines, late %lu lines (%lu records); held %lu records at the peak, kept %lu\n", (unsigned long)xr.n_early_lines,
		        (unsigned long)xr.n_late_lines, (unsigned long)xr.n_late_records, (unsigned long)xr.peak_records, (unsigned long)info.n_hits);
	if (no_cont) {
		if (ma_verbose >= 3) fprintf(MA_LOG, "[M::%s::%s] dropped %d contained reads\n", "ma_hit_no_cont", sys_timestamp(), info.n_excl);
		fprintf(MA_LOG, "[M::%s] ===> Step 1: reading read mappings <===\n", "main");
	}
	ingest_dictionary(c, &info, d, n_hits, 1, t0);
	return 0;
}

/* returns 0 and leaves the unsorted records in the context (as after mahip_hits_upload); -1 = could not open;
 * -2 = the device-side stage could not run (memory): the caller may use the host reader, which opens the file again (input that cannot be read twice -- stdin,
 * a pipe -- and was being streamed when the device refused is an error of the run instead) */
int ma_hit_ingest_gpu(mahip_ctx_t *c, const char *fn, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir)
{
	return ma_hit_ingest_gpu_excl(c, fn, min_span, min_match, d, n_hits, bi_dir, 0, 0, 0.f);
}

int ma_hit_ingest_gpu_excl(mahip_ctx_t *c, const char *fn, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int no_cont, int max_hang, float int_frac)
{
	const int timing = ma_timing_level() >= 1, mode = ma_ingest_stream_mode();
	double t0 = sys_realtime();
	{
		gzFile fp = 0;
		int seekable = 0;
		/* -R streams only under MA_STREAM_NOCONT=1 (the one-pass exclusion of mahip_paf_stream_begin_excl; measured in DESIGN 7, the default stays off); a rank of several never does */
		int rc = paf_load_ladder(c, fn, (!no_cont || ma_stream_nocont()) && mode != 0 && !mahip_comm_active(c) ? &fp : 0, &seekable, mode == 1);
		if (rc == 1) { /* the last rung, piece by piece */
			rc = ma_hit_ingest_stream_excl(c, fp, min_span, min_match, d, n_hits, bi_dir, ma_ingest_piece(), no_cont, max_hang, int_frac);
			gzclose(fp);
			if (rc == -2 && !seekable) {
				fprintf(stderr, "[E::%s] the device refused a piece of the input (%s), and what was read of it cannot be read again\n", __func__, mahip_strerror());
				exit(1);
			}
			return rc;
		}
		if (rc != 0) return rc; /* -1 cannot open, -2 does not fit */
	}
	if (timing) fprintf(stderr, "[T::ingest_gpu] load %.3f s\n", sys_realtime() - t0);
	return ma_hit_ingest_loaded_excl(c, min_span, min_match, d, n_hits, bi_dir, 1, no_cont, max_hang, int_frac);
}
