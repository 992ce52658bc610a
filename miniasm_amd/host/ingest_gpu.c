/* ingest_gpu.c -- the text part of ma_hit_read (reference hit.c:70-101, paf.c, sdict.c) on the device.
 *
 * The host only moves bytes: a plain file goes from the page cache straight into pinned staging slots and on to
 * HBM (mahip_paf_load_fd); a bgzip-compressed (BGZF) file goes to HBM as it is and is inflated there, one wave per block (mahip_bgzf_load_fd; the walk over
 * its member chain is below); a plain gzip file can be cut into chunks and inflated there too (MA_GZIP_DEVICE=1: mahip_gzip_load_fd; its header and trailer are
 * read below); otherwise gzip / stdin input is inflated into memory first (zlib, as the reference does through gzread) and uploaded.  Lines, columns, numbers, the span/match filter, the name dictionary with the reference's
 * first-appearance ids and the (mirrored) hit records are all produced by csrc/paf.hip; what comes back is the
 * dictionary (names + first-seen lengths, R entries) and, only for the per-symbol ABI, the records.
 * The -R pre-filter (ma_hit_no_cont, hit.c:38-68) rides in the same parse: the exclusion is a flag per name.
 * MA_HOST_PARSE=1 forces the host reader (ingest_mt.c / paf_reader.c); both are pinned to the same records and ids.
 */
#include <fcntl.h>
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

/* ---- plain gzip: the header and the trailer of the FIRST member (RFC 1952); whether it is the only one the device finds out (include/mahip.h).
 * returns MAHIP_GZIP_OK (*hdr_len = where the deflate stream starts; the trailer's CRC32 and ISIZE) or MAHIP_GZIP_BAD_HEADER; -1 on a read error */
int ma_gzip_head(int fd, const void *mem, uint64_t nbytes, uint64_t *hdr_len, uint32_t *crc, uint32_t *isize)
{
	bg_src_t src;
	unsigned char h[12], b[8];
	uint64_t p = 10;
	int k;
	memset(&src, 0, sizeof(src));
	src.fd = fd; src.mem = (const unsigned char*)mem; src.n = nbytes;
	*hdr_len = 0; *crc = *isize = 0;
	if (nbytes < 10 + 8) return MAHIP_GZIP_BAD_HEADER;
	if (bg_get(&src, 0, 10, h) != 0) return -1;
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
	if (bg_get(&src, nbytes - 8, 8, b) != 0) return -1;
	*hdr_len = p; *crc = bg_le32(b); *isize = bg_le32(b + 4);
	return MAHIP_GZIP_OK;
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

/* parse the text already loaded into the context (mahip_paf_load_*): records stay on the device, the dictionary is
 * rebuilt in d (which must be empty or a previous result of this function); release = free the text afterwards */
int ma_hit_ingest_loaded(mahip_ctx_t *c, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int release)
{
	return ma_hit_ingest_loaded_excl(c, min_span, min_match, d, n_hits, bi_dir, release, 0, 0, 0.f);
}

/* no_cont: -R, the reference's Step 0 (hit.c:38-68) folded into the same parse; prints its log line first */
int ma_hit_ingest_loaded_excl(mahip_ctx_t *c, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int release, int no_cont, int max_hang, float int_frac)
{
	const int timing = ma_timing_level() >= 1;
	double t1 = sys_realtime(), t2, t3;
	mahip_paf_info_t info;
	size_t tot_len = 0;
	GPU(mahip_set_shard(c, 0, 0xffffffffu));
	GPU_SOFT(mahip_paf_parse_excl(c, min_span, min_match, bi_dir, no_cont, max_hang, int_frac, &info));
	if (no_cont) {
		if (ma_verbose >= 3) fprintf(MA_LOG, "[M::%s::%s] dropped %d contained reads\n", "ma_hit_no_cont", sys_timestamp(), info.n_excl);
		fprintf(MA_LOG, "[M::%s] ===> Step 1: reading read mappings <===\n", "main");
	}
	t2 = sys_realtime();
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
	return 0;
}

/* file -> HBM; 0 ok, -1 = could not open */
int ma_paf_load_file(mahip_ctx_t *c, const char *fn)
{
	int fd = -1, is_plain = 0, is_reg = 0;
	struct stat st;
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
				if (bi.reason == MAHIP_BGZF_NOT_BGZF) { /* plain gzip: one deflate stream, cut into chunks on the device (include/mahip.h); any reason leaves it to zlib */
					mahip_gzip_info_t gi;
					if (!ma_gzip_device_enabled()) {
						memset(&gi, 0, sizeof(gi));
						gi.reader = MAHIP_BGZF_HOST; gi.reason = MAHIP_GZIP_FORCED; gi.first_bad_item = -1; gi.comp_bytes = (uint64_t)st.st_size;
						mahip_gzip_note(c, &gi);
						if (ma_timing_level() >= 1) fprintf(stderr, "[T::gzip] reader=host reason=%d (%s) item=-1 chunks=0 items=0\n", gi.reason, mahip_gzip_reason_name(gi.reason));
					} else {
						if (mahip_gzip_load_fd(c, fd, (size_t)st.st_size, MAHIP_BGZF_PAF, 0, &gi) != 0) { close(fd); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
						if (gi.reason == MAHIP_GZIP_OK) { close(fd); return 0; }
					}
				}
			}
		}
		fp = fd >= 0 ? gzdopen(fd, "r") : gzdopen(fileno(stdin), "r");
		size_t len = 0;
		char *buf;
		if (fp == 0) { if (fd >= 0) close(fd); return -1; }
		gzbuffer(fp, 1u << 20);
		buf = slurp_gz(fp, &len);
		gzclose(fp);
		if (mahip_paf_load_mem(c, buf, len) != 0) { free(buf); fprintf(stderr, "[W::%s] device-side parse not possible (%s); using the host reader\n", __func__, mahip_strerror()); mahip_paf_release(c); return -2; }
		free(buf);
	}
	return 0;
}

/* returns 0 and leaves the unsorted records in the context (as after mahip_hits_upload); -1 = could not open;
 * -2 = the device-side stage could not run (memory): nothing was consumed, the caller may use the host reader */
int ma_hit_ingest_gpu(mahip_ctx_t *c, const char *fn, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir)
{
	return ma_hit_ingest_gpu_excl(c, fn, min_span, min_match, d, n_hits, bi_dir, 0, 0, 0.f);
}

int ma_hit_ingest_gpu_excl(mahip_ctx_t *c, const char *fn, int min_span, int min_match, sdict_t *d, size_t *n_hits, int bi_dir, int no_cont, int max_hang, float int_frac)
{
	const int timing = ma_timing_level() >= 1;
	double t0 = sys_realtime();
	{
		int rc = ma_paf_load_file(c, fn);
		if (rc != 0) return rc; /* -1 cannot open, -2 does not fit */
	}
	if (timing) fprintf(stderr, "[T::ingest_gpu] load %.3f s\n", sys_realtime() - t0);
	return ma_hit_ingest_loaded_excl(c, min_span, min_match, d, n_hits, bi_dir, 1, no_cont, max_hang, int_frac);
}
