/* ingest_sharded.c -- the text part of ma_hit_read (reference hit.c:70-101, paf.c:34-67, sdict.c:27-45) on N GPUs, every rank on its own
 * byte range of the file ("ingest routing, option B"; the round-3 review's What's missing #2).
 *
 * Round 3 had every rank of `MA_GPUS=N miniasm` load and parse the WHOLE text and then keep the hits of its read range: N x the file through one
 * host's page cache, N full parses -- the command's end-to-end time could not shrink with N.  Here rank g reads the bytes [g S/N, (g+1) S/N), cut at
 * line starts (a rank's range begins behind the first newline at or after its nominal start; the line that straddles a border belongs to the rank
 * it starts in), parses them on its GPU, and the ranks exchange only what the reference's sequential reader carries across a border
 * (csrc/paf.hip: paf_cross_counts, paf_stale_bl, paf_dict_merged): line counts, the inherited `bl` of 10-column lines, the distinct names of each range with their first
 * appearances -- merged into one dictionary, the reference's ids, on every rank.  The records then travel to the ranks that own their query reads
 * in one personalised exchange (csrc/hits.hip: mahip_hits_route), each with its position in the input's record sequence, and the sharded head
 * (sharded.c) runs on ranks that hold their own records only.  Plain files only (a byte range of a gzip stream is not a text range); -R needs
 * the whole text on one rank: both fall back to the whole-text form.
 */
#define _GNU_SOURCE
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ma_host.h"

#define GPU(call) do { if ((call) != 0) ma_gpu_fail(__func__); } while (0)

/* first line start at or behind `at` (0 for at == 0; size when there is none): the byte behind the first '\n' in [at - 1, size) */
static off_t line_start_at(int fd, off_t at, off_t size)
{
	char buf[1 << 16];
	off_t pos;
	if (at <= 0) return 0;
	if (at >= size) return size;
	pos = at - 1; /* a newline right in front of `at` makes `at` itself a line start */
	while (pos < size) {
		ssize_t got = pread(fd, buf, sizeof(buf), pos), k;
		if (got <= 0) break;
		for (k = 0; k < got; ++k) if (buf[k] == '\n') return pos + k + 1 < size ? pos + k + 1 : size;
		pos += got;
	}
	return size;
}

/* 1 if `fn` can be ingested by ranges (a plain regular file), else 0 */
int ma_ingest_sharded_possible(const char *fn)
{
	struct stat st;
	unsigned char magic[2] = { 0, 0 };
	int fd, ok;
	if (fn == 0 || strcmp(fn, "-") == 0) return 0;
	fd = open(fn, O_RDONLY);
	if (fd < 0) return 0;
	ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && !(pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b);
	close(fd);
	return ok;
}

/* Collective over the context's communicator.  Afterwards: c holds this rank's OWN records (query read in its range) in input order with their positions,
 * the shard bounds are set, d holds the whole dictionary (every rank: the tail runs on rank 0, but the squeeze bookkeeping of the head wants n_seq
 * everywhere and the dictionary is two plain copies).  *n_hits_total / *n_lines: over all ranks.  Returns 0, -1 (cannot open), -2 (not possible: caller
 * falls back to the whole-text form on every rank -- decided from the file alone, so all ranks decide alike). */
int ma_hit_ingest_sharded(mahip_ctx_t *c, const char *fn, int min_span, int min_match, sdict_t *d, size_t *n_hits_total, int bi_dir, ma_ingest_shard_info_t *si)
{
	const int world = mahip_comm_world(c), rank = mahip_comm_rank(c);
	const int timing = ma_timing_level() >= 1;
	double t0 = sys_realtime(), t1, t2, t3;
	mahip_paf_info_t info;
	struct stat st;
	off_t beg, end;
	uint64_t n_total = 0, sent = 0, sums[2];
	int fd;
	if (!ma_ingest_sharded_possible(fn)) return -2;
	fd = open(fn, O_RDONLY);
	if (fd < 0 || fstat(fd, &st) != 0) { if (fd >= 0) close(fd); return -1; }
	beg = line_start_at(fd, (off_t)((unsigned long long)st.st_size * (unsigned)rank / (unsigned)world), st.st_size);
	end = rank + 1 == world ? st.st_size : line_start_at(fd, (off_t)((unsigned long long)st.st_size * (unsigned)(rank + 1) / (unsigned)world), st.st_size);
	if (end < beg) end = beg;
	GPU(mahip_set_shard(c, 0, 0xffffffffu));
	GPU(mahip_paf_load_fd_range(c, fd, (size_t)beg, (size_t)(end - beg)));
	close(fd);
	t1 = sys_realtime();
	GPU(mahip_paf_parse_sharded(c, min_span, min_match, bi_dir, &info));
	t2 = sys_realtime();
	{ /* the dictionary: names in one block + the sd_seq_t records the device wrote for that block */
		char *names = (char*)malloc(info.name_bytes ? info.name_bytes : 1);
		sd_seq_t *seq = (sd_seq_t*)malloc(((size_t)info.n_seq + 1) * sizeof(sd_seq_t));
		uint64_t tl = 0;
		GPU(mahip_paf_seqs(c, names, seq, &tl));
		ma_sd_adopt(d, names, info.name_bytes, info.n_seq, seq);
		if (si) si->tot_len = tl;
	}
	GPU(mahip_hits_route(c, &n_total, &sent)); /* releases nothing of the text stage yet: the records it reads live in the context's own buffer */
	GPU(mahip_paf_release(c));
	t3 = sys_realtime();
	sums[0] = (uint64_t)(end - beg); sums[1] = sent;
	if (si) {
		si->bytes_own = (uint64_t)(end - beg); si->bytes_file = (uint64_t)st.st_size; si->n_lines = info.n_lines; si->n_records = info.n_records;
		si->n_hits_total = n_total; si->bytes_routed = sent; si->max_qs = info.max_qs;
	}
	if (timing) fprintf(stderr, "[T::ingest_gpu] rank %d of %d: bytes [%lld, %lld) of %lld; load %.3f  parse+merge %.3f  dictionary+route %.3f s (%lu lines in all, %lu of %lu records sent on)\n",
	                    rank, world, (long long)beg, (long long)end, (long long)st.st_size, t1 - t0, t2 - t1, t3 - t2, (unsigned long)info.n_lines, (unsigned long)(sent / 36), (unsigned long)info.n_hits);
	*n_hits_total = (size_t)n_total;
	(void)sums;
	return 0;
}
