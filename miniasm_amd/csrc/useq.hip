// useq.hip -- unitig sequences on the device (reference asm.c:216-290 ma_ug_seq): every read placed on a unitig contributes the
// first `len` bases of its kept interval (forward) or the reverse complement of its last `len` bases (reverse strand).
// A plain reads file in the regular form is read here, on the device (second half of this file).  Otherwise the host reads the
// FASTA/FASTQ records (gzip or stdin: a byte stream only one thread can inflate) and hands the bases of the PLACED reads over in batches; the placement itself is a byte gather: one block per read, coalesced 1-byte loads / stores,
// complement through a 128-entry table in LDS.  HBM-bound by construction (bytes in = bytes out); the unitig arena stays in
// HBM until the last batch and comes back once.
#include "mahip_internal.hpp"
#include "text_core.h"

struct UseqBufs {
	DevBuf arena, seq, jobs; size_t arena_bytes = 0;
	bool arena_kept = false; // mahip_useq_end(c, NULL): the finished arena stays in HBM for the device text writer
	// the reads file as text (second half of this file): the text, newline counts of the granules and their scan, line starts, FASTA header flags and their
	// scan, header line of every record, counters; the wanted reads, their names, hashes, the table over them and the record each of them takes
	DevBuf fx_text, fx_gcnt, fx_gpos, fx_ls, fx_hdr, fx_hpos, fx_recl, fx_ctr, fx_want, fx_wname, fx_whash, fx_tab, fx_win;
	size_t fx_n = 0; uint32_t fx_L = 0, fx_R = 0; int fx_format = 0; bool fx_loaded = false, fx_regular = false;
	mahip_useq_info_t last = {0, 0, 0, 0, 0, 0, 0};
	// the streamed reader: the window lives in fx_text; counters of a window, its match list, the names seen so far
	DevBuf fw_ctr, fw_list, fw_seen;
	bool fw_active = false, fw_ended = false; size_t fw_n_want = 0, fw_n = 0, fw_carry_off = 0, fw_carry = 0, fw_cap = 0; uint32_t fw_mask = 0; double fw_t_place = 0;
	mahip_useq_stream_report_t fw_rep = {};
	// the wanted table the lookup and the placement read: the uploaded one (fx_want, fx_wname) or the plan's (pl_want, the blob of mahip_text_names)
	const mahip_useq_want_t *w_want = nullptr; const unsigned char *w_names = nullptr;
	// the placement plan (third part of this file): unitig offsets and the tile sums of their scan, first member of every unitig, the members' low words and their
	// scan, per read its member count and its place, wanted flags and their scan, the wanted table, counters; hand-made unitigs and intervals of the stage entry
	DevBuf pl_uoff, pl_bsum, pl_moff, pl_low, pl_mscan, pl_cnt, pl_place, pl_flag, pl_pos, pl_want, pl_ctr, pl_un, pl_ulen, pl_mem, pl_sub;
	bool pl_valid = false, pl_ctx = false; // pl_ctx: made of the unitigs mahip_ug_gen left in the context (mahip_useq_plan), not of hand-made ones
	uint64_t pl_names_gen = 0, pl_bad = 0; const unsigned char *pl_blob = nullptr;
	mahip_useq_plan_info_t pl_info = {};
};
static void fx_drop(mahip_ctx *c, UseqBufs *b);

static UseqBufs *useq_bufs(mahip_ctx *c)
{
	if (!c->useq) c->useq = new UseqBufs();
	return (UseqBufs*)c->useq;
}

void useq_free(mahip_ctx *c)
{
	UseqBufs *b = (UseqBufs*)c->useq;
	if (!b) return;
	dev_free(c, b->arena); dev_free(c, b->seq); dev_free(c, b->jobs);
	DevBuf *plan[] = {&b->pl_uoff, &b->pl_bsum, &b->pl_moff, &b->pl_low, &b->pl_mscan, &b->pl_cnt, &b->pl_place, &b->pl_flag, &b->pl_pos, &b->pl_want, &b->pl_ctr, &b->pl_un, &b->pl_ulen, &b->pl_mem, &b->pl_sub};
	for (DevBuf *d : plan) dev_free(c, *d);
	fx_drop(c, b);
	delete b;
	c->useq = nullptr;
}

// the reference's complement table (asm.c:225-234): IUPAC letters in both cases, everything else maps to itself, 0x60 to 0x40
__device__ __forceinline__ unsigned char comp_of(unsigned c)
{
	const char *from = "ABCDGHKMRTUVYabcdghkmrtuvy", *to = "TVGHCDMKYAABRtvghcdmkyaabr";
	if (c == 0x60) return 0x40;
	for (int k = 0; k < 26; ++k) if ((unsigned char)from[k] == c) return (unsigned char)to[k];
	return (unsigned char)c;
}

__global__ __launch_bounds__(256) void k_useq_gather(const unsigned char *__restrict__ seq, const mahip_useq_job_t *__restrict__ jobs, size_t n_jobs, unsigned char *__restrict__ arena)
{
	__shared__ unsigned char s_comp[128];
	if (threadIdx.x < 128) s_comp[threadIdx.x] = comp_of(threadIdx.x);
	__syncthreads();
	for (size_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
		const mahip_useq_job_t jb = jobs[j];
		const unsigned char *src = seq + jb.src_off;
		unsigned char *dst = arena + jb.dst_off;
		// a read file that disagrees with the PAF may hold fewer bases than the unitig takes from the read: the reference then reads outside its
		// buffer (asm.c:279-285, undefined); here those positions keep the arena's 'N' and nothing outside the batch is touched
		const uint32_t len = jb.len < jb.src_len ? jb.len : jb.src_len;
		if (!jb.rev) for (uint32_t i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
		else for (uint32_t i = threadIdx.x; i < len; i += 256) { const unsigned ch = src[jb.src_len - 1 - i]; dst[i] = ch >= 128 ? 'N' : s_comp[ch]; } // asm.c:283-285
	}
}

extern "C" int mahip_useq_begin(mahip_ctx_t *c, size_t arena_bytes)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	CHK(dev_reserve(c, b->arena, arena_bytes + 64));
	b->arena_bytes = arena_bytes; b->arena_kept = false;
	if (arena_bytes) HIPCHK(hipMemsetAsync(b->arena.p, 'N', arena_bytes, c->st)); // asm.c:246: positions no read covers stay 'N'
	return 0;
}

extern "C" int mahip_useq_batch(mahip_ctx_t *c, const char *h_seq, size_t seq_bytes, const mahip_useq_job_t *h_jobs, size_t n_jobs)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (n_jobs == 0) return 0;
	CHK(dev_reserve(c, b->seq, seq_bytes + 64)); CHK(dev_reserve(c, b->jobs, n_jobs * sizeof(mahip_useq_job_t)));
	CHK(xfer_copy(c, b->seq.p, (void*)h_seq, seq_bytes, 1));
	HIPCHK(hipMemcpyAsync(b->jobs.p, h_jobs, n_jobs * sizeof(mahip_useq_job_t), hipMemcpyHostToDevice, c->st));
	ProfScope ps(c, "k_useq_gather", 0);
	hipLaunchKernelGGL(k_useq_gather, dim3(grid_for(n_jobs, 1, 65536)), dim3(256), 0, c->st, (const unsigned char*)b->seq.p, (const mahip_useq_job_t*)b->jobs.p, n_jobs, (unsigned char*)b->arena.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->st)); // the host reuses h_seq / h_jobs for the next batch
	return 0;
}

extern "C" int mahip_useq_end(mahip_ctx_t *c, char *h_arena)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!h_arena) { b->arena_kept = true; return 0; } // no download: the placement is queued on the context's stream, and so is everything that reads the arena
	if (b->arena_bytes) CHK(xfer_copy(c, b->arena.p, h_arena, b->arena_bytes, 0));
	return 0;
}

bool useq_dev_arena(mahip_ctx *c, const char **arena, size_t *bytes)
{
	UseqBufs *b = (UseqBufs*)c->useq;
	if (!b || !b->arena_kept) return false;
	*arena = (const char*)b->arena.p; *bytes = b->arena_bytes;
	return true;
}

// ================================================================================================ the reads file on the device
// FASTA/FASTQ text in HBM -> line index -> form check -> name lookup -> placement straight from the text ("reads file").
// The reference's reader (kseq.h:192-232) is sequential in general: the quality length is defined by the sequence length, and '@', '+', '>' may begin a
// quality line.  Here the device VERIFIES that the file is in a form where the line index alone fixes the record structure and where kseq reads the same
// records (the "regular form", see mahip.h); anything else is reported with a reason and the caller keeps its host reader.
//   FASTA: first byte '>'; every line beginning with '>' is a header (kseq.h:209/214), every other non-empty line is a sequence line (kseq.h:211-212) and
//          must not begin with '@' or '+' (they end the sequence loop, kseq.h:209); empty lines are skipped (kseq.h:210).
//   FASTQ: four lines a record: '@' header, a sequence line that begins with none of '>' '@' '+', a '+' line (kseq.h:226 skips it), a quality line of
//          exactly the sequence's length (kseq.h:228 reads ONE line then and stops; any other length makes kseq_read return -2 at kseq.h:230, or makes it
//          read on into the next record).
//   no '\r' anywhere (kseq.h:146 drops one only from lines longer than 1).
#define FX_GRAN 1024u
#define FX_LONG_LINE ((uint64_t)1 << 24) // 256 lines shorter than this: their bases sum up in 32 bits (k_fx_place)
enum { FX_NL = 0, FX_CR, FX_FIRST, FX_LAST, FX_V_FASTA, FX_V_SHAPE, FX_V_QUAL, FX_MATCH, FX_DISTINCT, FX_SHORT, FX_NUL, FX_V_LONG, FX_NCTR = 16 };

struct FxText { const unsigned char *t; const uint64_t *ls; const uint32_t *recl; uint64_t n; uint32_t L, R; int fq; };

// bit 7 of every byte of w that equals the byte repeated in pat
__device__ __forceinline__ uint32_t fx_eq(uint32_t w, uint32_t pat) { const uint32_t x = w ^ pat; return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
// 16 bytes at off (a multiple of 16); bytes behind the text read as 0xff (none of the bytes that are counted)
__device__ __forceinline__ uint4 fx_load16(const unsigned char *__restrict__ t, uint64_t n, uint64_t off)
{
	if (off + 16 <= n) return *(const uint4*)(t + off);
	uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
	for (uint32_t k = 0; k < 16 && off + k < n; ++k) w[k >> 2] ^= (uint32_t)(t[off + k] ^ 0xffu) << (8 * (k & 3));
	return make_uint4(w[0], w[1], w[2], w[3]);
}

// one wave per 1 KiB granule: cnt[g] = its newlines; totals of '\n', '\r' and NUL; the first and the last byte of the text
__global__ __launch_bounds__(256) void k_fx_census(const unsigned char *__restrict__ t, uint64_t n, uint32_t n_gran, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr)
{
	const uint32_t lane = threadIdx.x & 63, n_waves = gridDim.x * 4u;
	uint64_t nl = 0, cr = 0, nul = 0;
	for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < n_gran; g += n_waves) { // the whole wave
		const uint4 v = fx_load16(t, n, (uint64_t)g * FX_GRAN + lane * 16u);
		const uint32_t a = (uint32_t)(__popc(fx_eq(v.x, 0x0a0a0a0au)) + __popc(fx_eq(v.y, 0x0a0a0a0au)) + __popc(fx_eq(v.z, 0x0a0a0a0au)) + __popc(fx_eq(v.w, 0x0a0a0a0au)));
		cr += (uint32_t)(__popc(fx_eq(v.x, 0x0d0d0d0du)) + __popc(fx_eq(v.y, 0x0d0d0d0du)) + __popc(fx_eq(v.z, 0x0d0d0d0du)) + __popc(fx_eq(v.w, 0x0d0d0d0du)));
		nul += (uint32_t)(__popc(fx_eq(v.x, 0u)) + __popc(fx_eq(v.y, 0u)) + __popc(fx_eq(v.z, 0u)) + __popc(fx_eq(v.w, 0u)));
		const uint32_t s = wv_sum_u32(a);
		if (lane == 0) cnt[g] = s;
		nl += a;
	}
	blk_add_u64(ctr + FX_NL, nl);
	blk_add_u64(ctr + FX_CR, cr);
	blk_add_u64(ctr + FX_NUL, nul);
	if (blockIdx.x == 0 && threadIdx.x == 0) { ctr[FX_FIRST] = t[0]; ctr[FX_LAST] = t[n - 1]; }
}

// ls[i] = offset of the first byte of line i; line i is bytes [ls[i], ls[i + 1] - 1).  ls[L] = n behind a final newline, n + 1 without one.
__global__ __launch_bounds__(256) void k_fx_lines(const unsigned char *__restrict__ t, uint64_t n, uint32_t n_gran, const uint32_t *__restrict__ gpos, uint32_t L, uint64_t *__restrict__ ls)
{
	const uint32_t lane = threadIdx.x & 63, n_waves = gridDim.x * 4u;
	for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < n_gran; g += n_waves) { // the whole wave
		const uint64_t off = (uint64_t)g * FX_GRAN + lane * 16u;
		const uint4 v = fx_load16(t, n, off);
		const uint32_t m[4] = {fx_eq(v.x, 0x0a0a0a0au), fx_eq(v.y, 0x0a0a0a0au), fx_eq(v.z, 0x0a0a0a0au), fx_eq(v.w, 0x0a0a0a0au)};
		const uint32_t a = (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
		uint32_t at = gpos[g] + (uint32_t)wv_scan_incl_i32((int)a, lane) - a + 1u; // line that starts behind this lane's first newline
		if (a) for (uint32_t k = 0; k < 16; ++k) if (m[k >> 2] >> (8 * (k & 3) + 7) & 1u) ls[at++] = off + k + 1;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) { ls[0] = 0; if (t[n - 1] != '\n') ls[L] = n + 1; }
}

__device__ __forceinline__ uint32_t fx_first(const FxText &x, uint32_t i) { const uint64_t b = x.ls[i]; return x.ls[i + 1] - 1 > b ? x.t[b] : 0u; } // 0: an empty line

// FASTA: header flags, the lines that may not be there, and lines of FX_LONG_LINE bytes or more in a record of several lines (the whole block calls it)
__device__ __forceinline__ void fx_form_fasta_lines(const FxText &x, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ ctr)
{
	uint64_t bad = 0, lng = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < x.L; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t ch = fx_first(x, (uint32_t)i);
		hdr[i] = ch == '>';
		bad += ch == '@' || ch == '+';
		if (ch != '>' && x.ls[i + 1] - 1 - x.ls[i] >= FX_LONG_LINE) // (line 0 is a header) fine as the only line of its record: that one is copied without a scan
			lng += fx_first(x, (uint32_t)i - 1) != '>' || (i + 1 < x.L && fx_first(x, (uint32_t)i + 1) != '>');
	}
	blk_add_u64(ctr + FX_V_FASTA, bad);
	blk_add_u64(ctr + FX_V_LONG, lng);
}
__global__ __launch_bounds__(256) void k_fx_form_fasta(const FxText x, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ ctr) { fx_form_fasta_lines(x, hdr, ctr); }
// recl[r] = header line of record r, recl[R] = L
__global__ __launch_bounds__(256) void k_fx_rec_lines(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ hpos, uint32_t L, uint32_t *__restrict__ recl)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < L; i += (uint64_t)gridDim.x * 256u) if (hdr[i]) recl[hpos[i]] = (uint32_t)i;
	if (blockIdx.x == 0 && threadIdx.x == 0) recl[hpos[L]] = L;
}
// FASTQ: record r = lines 4r .. 4r + 3 (the whole block calls it)
__device__ __forceinline__ void fx_form_fastq_records(const FxText &x, unsigned long long *__restrict__ ctr)
{
	uint64_t shape = 0, qual = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < x.R; r += (uint64_t)gridDim.x * 256u) {
		const uint32_t i = (uint32_t)r * 4u, c0 = fx_first(x, i), c1 = fx_first(x, i + 1), c2 = fx_first(x, i + 2);
		shape += c0 != '@' || c1 == '>' || c1 == '@' || c1 == '+' || c2 != '+';
		qual += x.ls[i + 2] - x.ls[i + 1] != x.ls[i + 4] - x.ls[i + 3];
	}
	blk_add_u64(ctr + FX_V_SHAPE, shape);
	blk_add_u64(ctr + FX_V_QUAL, qual);
}
__global__ __launch_bounds__(256) void k_fx_form_fastq(const FxText x, unsigned long long *__restrict__ ctr) { fx_form_fastq_records(x, ctr); } // (L is a multiple of 4)

// record r: its header line, its sequence lines [*j0, *j1) and the bases they hold (every line of the stretch ends with one byte that is not a base)
__device__ __forceinline__ uint32_t fx_record(const FxText &x, uint32_t r, uint32_t *j0, uint32_t *j1, uint64_t *nb)
{
	const uint32_t h = x.fq ? r * 4u : x.recl[r];
	*j0 = h + 1; *j1 = x.fq ? h + 2 : x.recl[r + 1];
	*nb = x.ls[*j1] - x.ls[*j0] - (*j1 - *j0);
	return h;
}
// the name: the header's bytes behind the marker up to the first white space (kseq.h:203, isspace without '\r' and with the line end as the limit)
__device__ __forceinline__ uint32_t fx_name(const FxText &x, uint32_t h, uint64_t *off)
{
	const uint64_t b = x.ls[h] + 1, e = x.ls[h + 1] - 1;
	uint64_t p = b;
	for (; p < e; ++p) { const unsigned ch = x.t[p]; if (ch == ' ' || ch == '\t' || ch == '\v' || ch == '\f') break; }
	*off = b;
	return (uint32_t)(p - b);
}
__device__ __forceinline__ uint64_t fx_hash(const unsigned char *s, uint32_t l)
{ // FNV-1a, 64 bits
	uint64_t h = 0xcbf29ce484222325ull;
	for (uint32_t k = 0; k < l; ++k) h = (h ^ s[k]) * 0x100000001b3ull;
	return h;
}
__global__ __launch_bounds__(256) void k_fx_name_spans(const FxText x, uint64_t *__restrict__ off, uint32_t *__restrict__ len)
{
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < x.R; r += (uint64_t)gridDim.x * 256u) {
		uint32_t j0, j1; uint64_t nb;
		len[r] = fx_name(x, fx_record(x, (uint32_t)r, &j0, &j1, &nb), &off[r]);
	}
}

// the wanted reads (distinct names) into an open-addressing table: tab[slot] = index + 1, linear probing
__global__ __launch_bounds__(256) void k_fx_tab_build(const mahip_useq_want_t *__restrict__ want, const unsigned char *__restrict__ wname, uint32_t n_want, uint64_t *__restrict__ whash,
                                                      uint32_t *__restrict__ tab, uint32_t mask)
{
	for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < n_want; w += gridDim.x * 256u) {
		const uint64_t h = fx_hash(wname + want[w].name_off, want[w].name_len);
		whash[w] = h;
		uint32_t s = (uint32_t)h & mask;
		while (atomicCAS(&tab[s], 0u, w + 1u) != 0u) s = (s + 1u) & mask;
	}
}
// record r's name against the table: the wanted read that carries it + 1 (0: none), and the bases the record holds
__device__ __forceinline__ uint32_t fx_lookup(const FxText &x, uint32_t r, const mahip_useq_want_t *__restrict__ want, const unsigned char *__restrict__ wname, const uint64_t *__restrict__ whash,
                                              const uint32_t *__restrict__ tab, uint32_t mask, uint64_t *nb)
{
	uint32_t j0, j1; uint64_t off;
	const uint32_t l = fx_name(x, fx_record(x, r, &j0, &j1, nb), &off);
	if (l == 0) return 0; // an empty name matches nothing
	const unsigned char *s = x.t + off;
	const uint64_t h = fx_hash(s, l);
	for (uint32_t p = (uint32_t)h & mask;; p = (p + 1u) & mask) {
		const uint32_t e = tab[p];
		if (e == 0) return 0;
		if (whash[e - 1] != h || want[e - 1].name_len != l) continue;
		const unsigned char *q = wname + want[e - 1].name_off;
		uint32_t k = 0;
		while (k < l && q[k] == s[k]) ++k;
		if (k == l) return e;
	}
}
// every record's name against the table; a wanted read keeps the LAST record that carries its name (the reference's loop overwrites, asm.c:262-284)
__global__ __launch_bounds__(256) void k_fx_probe(const FxText x, const mahip_useq_want_t *__restrict__ want, const unsigned char *__restrict__ wname, const uint64_t *__restrict__ whash,
                                                  const uint32_t *__restrict__ tab, uint32_t mask, uint32_t *__restrict__ win, unsigned long long *__restrict__ ctr)
{
	uint64_t n_match = 0, n_distinct = 0, n_short = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < x.R; r += (uint64_t)gridDim.x * 256u) {
		uint64_t nb;
		const uint32_t e = fx_lookup(x, (uint32_t)r, want, wname, whash, tab, mask, &nb);
		if (e == 0) continue;
		++n_match;
		n_distinct += atomicMax(&win[e - 1], (uint32_t)r + 1u) == 0u;
		n_short += nb < (uint64_t)(want[e - 1].whole ? want[e - 1].len : want[e - 1].e);
	}
	blk_add_u64(ctr + FX_MATCH, n_match);
	blk_add_u64(ctr + FX_DISTINCT, n_distinct);
	blk_add_u64(ctr + FX_SHORT, n_short);
}

// the per-read body of the placement (the whole block calls it): the bases of record `rec` from the text into the arena, forward or reverse complement as
// k_useq_gather does it.  A sequence on one line (FASTQ, unwrapped FASTA) is a straight coalesced copy; a wrapped one goes through 256 lines at a time: their
// lengths are scanned into base offsets in LDS and every base finds its line by a binary search there (8 steps), so consecutive lanes still read consecutive
// bytes except at the line ends.
struct FxPlaceLds { unsigned char comp[128]; uint64_t start[256]; uint32_t off[256], wave[4]; };
__device__ __forceinline__ void fx_place_read(const FxText &x, const mahip_useq_want_t &wt, uint32_t rec, unsigned char *__restrict__ arena, FxPlaceLds &m)
{
	uint32_t j0, j1; uint64_t nb;
	fx_record(x, rec, &j0, &j1, &nb);
	const uint64_t s = wt.whole ? 0 : wt.s, e = wt.whole ? nb : wt.e; // the kept interval [s, e) of the read's bases (the caller made sure that nb >= e)
	const uint64_t len = wt.len < e - s ? wt.len : e - s;
	const uint64_t lo = wt.rev ? e - len : s, hi = lo + len;          // the bases that are placed
	unsigned char *dst = arena + wt.dst_off;
	if (j1 - j0 == 1) {
		const unsigned char *src = x.t + x.ls[j0];
		if (!wt.rev) for (uint64_t i = threadIdx.x; i < len; i += 256) dst[i] = src[s + i];
		else for (uint64_t i = threadIdx.x; i < len; i += 256) { const unsigned ch = src[e - 1 - i]; dst[i] = ch >= 128 ? 'N' : m.comp[ch]; } // asm.c:280-281
		return;
	}
	uint64_t run = 0; // bases in front of the chunk
	for (uint32_t cj = j0; cj < j1 && run < hi; cj += 256) {
		const uint32_t cnt = j1 - cj < 256u ? j1 - cj : 256u, j = cj + threadIdx.x;
		uint32_t tot;
		const uint32_t ll = threadIdx.x < cnt ? (uint32_t)(x.ls[j + 1] - x.ls[j] - 1) : 0u;
		const uint32_t ex = block_excl_scan_256(ll, m.wave, &tot);
		if (threadIdx.x < cnt) { m.start[threadIdx.x] = x.ls[j]; m.off[threadIdx.x] = ex; }
		__syncthreads();
		const uint64_t b0 = lo > run ? lo : run, b1 = hi < run + tot ? hi : run + tot;
		for (uint64_t b = b0 + threadIdx.x; b < b1; b += 256) {
			const uint32_t rel = (uint32_t)(b - run);
			uint32_t ka = 0, kb = cnt; // the last line of the chunk that starts at or in front of the base
			while (kb - ka > 1) { const uint32_t mid = (ka + kb) >> 1; if (m.off[mid] <= rel) ka = mid; else kb = mid; }
			const unsigned ch = x.t[m.start[ka] + (rel - m.off[ka])];
			if (!wt.rev) dst[b - s] = (unsigned char)ch;
			else dst[e - 1 - b] = ch >= 128 ? 'N' : m.comp[ch];
		}
		run += tot;
		__syncthreads();
	}
}
// one block per wanted read (the whole-file reader: once per file)
__global__ __launch_bounds__(256) void k_fx_place(const FxText x, const mahip_useq_want_t *__restrict__ want, uint32_t n_want, const uint32_t *__restrict__ win, unsigned char *__restrict__ arena)
{
	__shared__ FxPlaceLds m;
	if (threadIdx.x < 128) m.comp[threadIdx.x] = comp_of(threadIdx.x);
	__syncthreads();
	for (uint32_t w = blockIdx.x; w < n_want; w += gridDim.x) { // the whole block
		const uint32_t rec = win[w];
		if (rec == 0) continue; // not in the file: its positions stay 'N'
		fx_place_read(x, want[w], rec - 1, arena, m);
	}
}

// ------------------------------------------------------------------------------------------------ the same text a window at a time
// The streamed reader holds one WINDOW of the text: the carry (the bytes of the window before that did not yet form a complete record) and the next piece.  The
// census and the line index above run on the window as they are; the kernels below find the consumed prefix (FASTQ: lines 0 .. 4*floor(L/4) - 1; FASTA: the lines
// in front of the window's last header line; everything in the last window), number its records only and leave the carry in the counter block.  Everything that
// follows reads L and R of the PREFIX from that block, so the host reads counters twice a window (the line count, then everything else) and no launch is sized
// by, or sweeps, the wanted list: the probe appends the wanted reads that matched to a list, and the placement runs one block per entry of it.
enum { FXW_LASTHDR = 16, FXW_LC, FXW_R, FXW_CONSUMED, FXW_CARRY, FXW_NLIST, FXW_CR, FXW_NUL, FXW_NCTR = 32 };

__device__ __forceinline__ FxText fxw_prefix_view(FxText x, const unsigned long long *__restrict__ ctr) { x.L = (uint32_t)ctr[FXW_LC]; x.R = (uint32_t)ctr[FXW_R]; return x; }

// FASTA: header flags of every line of the window, and its last header line (+ 1)
__global__ __launch_bounds__(256) void k_fxw_hdr(const FxText x, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ ctr)
{
	uint64_t last = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < x.L; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t h = fx_first(x, (uint32_t)i) == '>';
		hdr[i] = h;
		if (h) last = i + 1;
	}
	blk_max_u64(ctr + FXW_LASTHDR, last);
}
// the consumed prefix: its lines, its records, its bytes, and what stays behind it (one thread; x.L = the lines of the window; hpos: FASTA only)
__global__ void k_fxw_prefix(const FxText x, const uint32_t *__restrict__ hpos, int last, unsigned long long *__restrict__ ctr)
{
	if (blockIdx.x || threadIdx.x) return;
	uint32_t Lc, R;
	if (x.fq) { Lc = last ? x.L : x.L & ~3u; R = x.L / 4u; }
	else { const uint32_t lh = (uint32_t)ctr[FXW_LASTHDR]; Lc = last ? x.L : lh ? lh - 1u : 0u; R = hpos[Lc]; }
	const uint64_t used = x.ls[Lc] < x.n ? x.ls[Lc] : x.n; // (ls[L] = n + 1 behind a last line without its newline)
	ctr[FXW_LC] = Lc; ctr[FXW_R] = R; ctr[FXW_CONSUMED] = used; ctr[FXW_CARRY] = x.n - used;
}
// recl[r] = header line of record r of the prefix, recl[R] = its line count
__global__ __launch_bounds__(256) void k_fxw_rec_lines(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ hpos, const unsigned long long *__restrict__ ctr, uint32_t *__restrict__ recl)
{
	const uint32_t Lc = (uint32_t)ctr[FXW_LC];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < Lc; i += (uint64_t)gridDim.x * 256u) if (hdr[i]) recl[hpos[i]] = (uint32_t)i;
	if (blockIdx.x == 0 && threadIdx.x == 0) recl[ctr[FXW_R]] = Lc;
}
// '\r' and NUL bytes of the prefix (one wave per granule, as the census)
__global__ __launch_bounds__(256) void k_fxw_bytes(const unsigned char *__restrict__ t, unsigned long long *__restrict__ ctr)
{
	const uint64_t n = ctr[FXW_CONSUMED];
	const uint32_t lane = threadIdx.x & 63, n_waves = gridDim.x * 4u, n_gran = (uint32_t)((n + FX_GRAN - 1) / FX_GRAN);
	uint64_t cr = 0, nul = 0;
	for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < n_gran; g += n_waves) {
		const uint4 v = fx_load16(t, n, (uint64_t)g * FX_GRAN + lane * 16u);
		cr += (uint32_t)(__popc(fx_eq(v.x, 0x0d0d0d0du)) + __popc(fx_eq(v.y, 0x0d0d0d0du)) + __popc(fx_eq(v.z, 0x0d0d0d0du)) + __popc(fx_eq(v.w, 0x0d0d0d0du)));
		nul += (uint32_t)(__popc(fx_eq(v.x, 0u)) + __popc(fx_eq(v.y, 0u)) + __popc(fx_eq(v.z, 0u)) + __popc(fx_eq(v.w, 0u)));
	}
	blk_add_u64(ctr + FXW_CR, cr);
	blk_add_u64(ctr + FXW_NUL, nul);
}
__global__ __launch_bounds__(256) void k_fxw_form_fasta(const FxText x, uint32_t *__restrict__ hdr, unsigned long long *__restrict__ ctr) { fx_form_fasta_lines(fxw_prefix_view(x, ctr), hdr, ctr); }
__global__ __launch_bounds__(256) void k_fxw_form_fastq(const FxText x, unsigned long long *__restrict__ ctr) { fx_form_fastq_records(fxw_prefix_view(x, ctr), ctr); }

// the probe of a window: as k_fx_probe, and the lane whose atomicMax found win[w] == 0 -- the first record of the window that carries the name -- appends w to the
// window's match list, one atomic per wave (ballot, popcount, one add by the first lane that has one, broadcast).  `seen` lives for the whole stream: a name
// counts as distinct only in the first window that holds it.  The loop is uniform for the wave: every lane is at the ballot.
__global__ __launch_bounds__(256) void k_fxw_probe(const FxText xw, const mahip_useq_want_t *__restrict__ want, const unsigned char *__restrict__ wname, const uint64_t *__restrict__ whash,
                                                   const uint32_t *__restrict__ tab, uint32_t mask, uint32_t *__restrict__ win, const unsigned char *__restrict__ seen, uint32_t *__restrict__ list,
                                                   unsigned long long *__restrict__ ctr)
{
	const FxText x = fxw_prefix_view(xw, ctr);
	const unsigned lane = threadIdx.x & 63;
	uint64_t n_match = 0, n_distinct = 0, n_short = 0;
	for (uint64_t r0 = (uint64_t)blockIdx.x * 256u; r0 < x.R; r0 += (uint64_t)gridDim.x * 256u) {
		const uint64_t r = r0 + threadIdx.x;
		uint64_t nb = 0;
		const uint32_t e = r < x.R ? fx_lookup(x, (uint32_t)r, want, wname, whash, tab, mask, &nb) : 0u;
		int first = 0;
		if (e) {
			++n_match;
			first = atomicMax(&win[e - 1], (uint32_t)r + 1u) == 0u;
			n_distinct += first && !seen[e - 1];
			n_short += nb < (uint64_t)(want[e - 1].whole ? want[e - 1].len : want[e - 1].e);
		}
		const uint64_t m = wv_ballot(first);
		if (m) {
			const int lead = __ffsll((long long)m) - 1;
			uint32_t base = 0;
			if (lane == (unsigned)lead) base = (uint32_t)atomicAdd(ctr + FXW_NLIST, (unsigned long long)__popcll(m));
			base = wv_bcast(base, lead);
			if (first) list[base + (uint32_t)__popcll(m & wv_lt(lane))] = e - 1;
		}
	}
	blk_add_u64(ctr + FX_MATCH, n_match);
	blk_add_u64(ctr + FX_DISTINCT, n_distinct);
	blk_add_u64(ctr + FX_SHORT, n_short);
}
// one block per entry of the match list: the copy of k_fx_place; then win[w] goes back to 0 -- win[] is all zero between windows without a sweep -- and the name is seen
__global__ __launch_bounds__(256) void k_fxw_place(const FxText x, const mahip_useq_want_t *__restrict__ want, const uint32_t *__restrict__ list, uint32_t n_list, uint32_t *__restrict__ win,
                                                   unsigned char *__restrict__ seen, unsigned char *__restrict__ arena)
{
	__shared__ FxPlaceLds m;
	if (threadIdx.x < 128) m.comp[threadIdx.x] = comp_of(threadIdx.x);
	__syncthreads();
	for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) { // the whole block
		const uint32_t w = list[k], rec = win[w];
		fx_place_read(x, want[w], rec - 1, arena, m);
		__syncthreads(); // every thread has read win[w]
		if (threadIdx.x == 0) { win[w] = 0; seen[w] = 1; }
	}
}
// the carry to the front of the window when the two stretches overlap: one block, ascending tiles of 4 KiB, every tile read whole before it is written (the
// destination lies in front of the source, so a tile's stores reach no byte that is still to be read)
__global__ __launch_bounds__(256) void k_fxw_move(unsigned char *__restrict__ t, uint64_t src, uint64_t n)
{
	for (uint64_t b = 0; b < n; b += 4096) {
		unsigned char v[16];
		const uint64_t at = b + threadIdx.x * 16u;
		for (uint32_t k = 0; k < 16; ++k) if (at + k < n) v[k] = t[src + at + k];
		__syncthreads();
		for (uint32_t k = 0; k < 16; ++k) if (at + k < n) t[at + k] = v[k];
		__syncthreads();
	}
}

static void fx_drop(mahip_ctx *c, UseqBufs *b)
{
	DevBuf *all[] = {&b->fx_text, &b->fx_gcnt, &b->fx_gpos, &b->fx_ls, &b->fx_hdr, &b->fx_hpos, &b->fx_recl, &b->fx_ctr, &b->fx_want, &b->fx_wname, &b->fx_whash, &b->fx_tab, &b->fx_win, &b->fw_ctr, &b->fw_list, &b->fw_seen};
	for (DevBuf *d : all) dev_free(c, *d);
	b->fx_n = 0; b->fx_loaded = b->fx_regular = false; b->fw_active = false;
	b->w_want = nullptr; b->w_names = nullptr;
}

static int fx_reserve_text(mahip_ctx *c, size_t nbytes)
{
	UseqBufs *b = useq_bufs(c);
	b->fx_loaded = b->fx_regular = false;
	if (nbytes == 0) { mahip_set_error("mahip_fastx_load: empty text"); return -1; }
	CHK(dev_reserve(c, b->fx_text, nbytes + 64));
	b->fx_n = nbytes;
	return 0;
}
int fx_text_reserve(mahip_ctx *c, size_t nbytes, void **d_text) { CHK(fx_reserve_text(c, nbytes)); *d_text = useq_bufs(c)->fx_text.p; return 0; }
void fx_text_loaded(mahip_ctx *c) { useq_bufs(c)->fx_loaded = true; }
extern "C" int mahip_fastx_load_mem(mahip_ctx_t *c, const void *text, size_t nbytes)
{
	HIPCHK(hipSetDevice(c->dev));
	CHK(fx_reserve_text(c, nbytes));
	CHK(xfer_copy(c, useq_bufs(c)->fx_text.p, (void*)text, nbytes, 1));
	useq_bufs(c)->fx_loaded = true;
	return 0;
}
extern "C" int mahip_fastx_load_fd(mahip_ctx_t *c, int fd, size_t nbytes)
{
	HIPCHK(hipSetDevice(c->dev));
	if (nbytes == 0) { mahip_set_error("mahip_fastx_load_fd: empty file"); return -1; }
	if (fx_reserve_text(c, nbytes) != 0) return 1; // no room for the text: the caller may read the file itself
	CHK(xfer_from_fd(c, useq_bufs(c)->fx_text.p, fd, nbytes));
	useq_bufs(c)->fx_loaded = true;
	return 0;
}
extern "C" int mahip_fastx_release(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	if (c->useq) { HIPCHK(hipStreamSynchronize(c->st)); fx_drop(c, (UseqBufs*)c->useq); }
	return 0;
}
extern "C" const char *mahip_fastx_reason_name(int reason)
{
	static const char *const nm[] = {"ok", "carriage returns in the file", "first byte is neither '>' nor '@'", "a FASTA sequence line begins with '@' or '+'", "FASTQ records are not four lines each",
	                                 "a FASTQ quality line differs in length from its sequence", "more than 2^32 - 1 lines", "not enough device memory", "a wanted read is shorter than its placement",
	                                 "not a plain file", "MA_FASTX_HOST is set", "NUL bytes in the file", "a line of 16 MiB or more in a wrapped FASTA record"};
	return reason >= 0 && reason < (int)(sizeof(nm) / sizeof(nm[0])) ? nm[reason] : "?";
}

static int fx_counters(mahip_ctx *c, UseqBufs *b, unsigned long long *h)
{
	HIPCHK(hipMemcpyAsync(h, b->fx_ctr.p, FX_NCTR * 8, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	return 0;
}
static FxText fx_view(UseqBufs *b)
{
	FxText x = {(const unsigned char*)b->fx_text.p, (const uint64_t*)b->fx_ls.p, (const uint32_t*)b->fx_recl.p, (uint64_t)b->fx_n, b->fx_L, b->fx_R, b->fx_format == MAHIP_FASTX_FASTQ};
	return x;
}

#define FX_RESERVE(buf, bytes) do { if (dev_reserve(c, (buf), (bytes)) != 0) { info->reason = MAHIP_FASTX_NOMEM; return 0; } } while (0)
extern "C" int mahip_fastx_index(mahip_ctx_t *c, mahip_fastx_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	memset(info, 0, sizeof(*info));
	if (!b->fx_loaded) { mahip_set_error("mahip_fastx_index: no text loaded"); return -1; }
	b->fx_regular = false;
	const uint64_t n = b->fx_n;
	const uint32_t n_gran = (uint32_t)((n + FX_GRAN - 1) / FX_GRAN);
	if ((n + FX_GRAN - 1) / FX_GRAN > 0xffffffffull) { info->reason = MAHIP_FASTX_TOO_MANY_LINES; return 0; }
	unsigned long long h[FX_NCTR];
	FX_RESERVE(b->fx_ctr, FX_NCTR * 8); FX_RESERVE(b->fx_gcnt, (size_t)n_gran * 4); FX_RESERVE(b->fx_gpos, (size_t)n_gran * 4 + 4);
	HIPCHK(hipMemsetAsync(b->fx_ctr.p, 0, FX_NCTR * 8, c->st));
	{
		ProfScope ps(c, "k_fx_census", (double)n);
		hipLaunchKernelGGL(k_fx_census, dim3(grid_for(n_gran, 4, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const unsigned char*)b->fx_text.p, n, n_gran, P<uint32_t>(b->fx_gcnt), P<unsigned long long>(b->fx_ctr));
		HIPCHK(hipGetLastError());
	}
	CHK(fx_counters(c, b, h));
	const uint64_t L = h[FX_NL] + (h[FX_LAST] != '\n');
	info->n_lines = L; info->n_cr = h[FX_CR];
	info->format = h[FX_FIRST] == '>' ? MAHIP_FASTX_FASTA : h[FX_FIRST] == '@' ? MAHIP_FASTX_FASTQ : 0;
	b->fx_format = info->format;
	if (info->n_cr) { info->reason = MAHIP_FASTX_CR; return 0; }
	if (h[FX_NUL]) { info->reason = MAHIP_FASTX_NUL_BYTE; return 0; } // the reference's names are C strings (asm.c:266): a name ends at a NUL for it
	if (info->format == 0) { info->reason = MAHIP_FASTX_FIRST_BYTE; return 0; }
	if (L > 0xffffffffull) { info->reason = MAHIP_FASTX_TOO_MANY_LINES; return 0; }
	b->fx_L = (uint32_t)L;
	FX_RESERVE(b->fx_ls, (size_t)(L + 2) * 8);
	CHK(scan_exclusive_u32(c, P<uint32_t>(b->fx_gcnt), P<uint32_t>(b->fx_gpos), n_gran, nullptr));
	{
		ProfScope ps(c, "k_fx_lines", (double)n + 8.0 * (double)L);
		hipLaunchKernelGGL(k_fx_lines, dim3(grid_for(n_gran, 4, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const unsigned char*)b->fx_text.p, n, n_gran, P<uint32_t>(b->fx_gpos), (uint32_t)L, P<uint64_t>(b->fx_ls));
		HIPCHK(hipGetLastError());
	}
	if (info->format == MAHIP_FASTX_FASTQ) {
		b->fx_R = (uint32_t)(L / 4);
		info->n_records = L / 4;
		if (L % 4) { info->reason = MAHIP_FASTX_FASTQ_SHAPE; return 0; }
		ProfScope ps(c, "k_fx_form_fastq", 40.0 * (double)b->fx_R);
		hipLaunchKernelGGL(k_fx_form_fastq, dim3(grid_for(b->fx_R, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, fx_view(b), P<unsigned long long>(b->fx_ctr));
		HIPCHK(hipGetLastError());
	} else {
		FX_RESERVE(b->fx_hdr, (size_t)L * 4); FX_RESERVE(b->fx_hpos, (size_t)(L + 1) * 4);
		{
			ProfScope ps(c, "k_fx_form_fasta", 20.0 * (double)L);
			hipLaunchKernelGGL(k_fx_form_fasta, dim3(grid_for(L, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, fx_view(b), P<uint32_t>(b->fx_hdr), P<unsigned long long>(b->fx_ctr));
			HIPCHK(hipGetLastError());
		}
		CHK(scan_exclusive_u32(c, P<uint32_t>(b->fx_hdr), P<uint32_t>(b->fx_hpos), L, P<uint32_t>(b->fx_hpos) + L));
		uint32_t R = 0;
		HIPCHK(hipMemcpyAsync(&R, P<uint32_t>(b->fx_hpos) + L, 4, hipMemcpyDeviceToHost, c->st));
		HIPCHK(hipStreamSynchronize(c->st));
		b->fx_R = R; info->n_records = R;
		FX_RESERVE(b->fx_recl, (size_t)(R + 1) * 4);
		ProfScope ps(c, "k_fx_rec_lines", 8.0 * (double)L);
		hipLaunchKernelGGL(k_fx_rec_lines, dim3(grid_for(L, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, P<uint32_t>(b->fx_hdr), P<uint32_t>(b->fx_hpos), (uint32_t)L, P<uint32_t>(b->fx_recl));
		HIPCHK(hipGetLastError());
	}
	CHK(fx_counters(c, b, h));
	if (h[FX_V_FASTA]) info->reason = MAHIP_FASTX_FASTA_LINE_START;
	else if (h[FX_V_SHAPE]) info->reason = MAHIP_FASTX_FASTQ_SHAPE;
	else if (h[FX_V_QUAL]) info->reason = MAHIP_FASTX_FASTQ_QUAL_LEN;
	else if (h[FX_V_LONG]) info->reason = MAHIP_FASTX_LONG_LINE;
	else { info->regular = 1; b->fx_regular = true; }
	return 0;
}
#undef FX_RESERVE

extern "C" int mahip_fastx_line_starts(mahip_ctx_t *c, uint64_t *out)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fx_loaded || !b->fx_ls.p) { mahip_set_error("mahip_fastx_line_starts: no line index"); return -1; }
	HIPCHK(hipMemcpyAsync(out, b->fx_ls.p, ((size_t)b->fx_L + 1) * 8, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	return 0;
}
extern "C" int mahip_fastx_name_spans(mahip_ctx_t *c, uint64_t *off, uint32_t *len)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fx_regular) { mahip_set_error("mahip_fastx_name_spans: the text is not in the regular form"); return -1; }
	const size_t R = b->fx_R;
	if (R == 0) return 0;
	DevBuf d_off, d_len;
	int rc = dev_reserve(c, d_off, R * 8) || dev_reserve(c, d_len, R * 4);
	if (rc == 0) {
		hipLaunchKernelGGL(k_fx_name_spans, dim3(grid_for(R, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, fx_view(b), P<uint64_t>(d_off), P<uint32_t>(d_len));
		rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(off, d_off.p, R * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
		     hipMemcpyAsync(len, d_len.p, R * 4, hipMemcpyDeviceToHost, c->st) != hipSuccess;
		if (hipStreamSynchronize(c->st) != hipSuccess) rc = 1;
		if (rc) mahip_set_error("mahip_fastx_name_spans: launch or copy failed");
	}
	dev_free(c, d_off); dev_free(c, d_len);
	return rc ? -1 : 0;
}

static double fx_now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + ts.tv_nsec * 1e-9; }

// the table over the wanted reads b->w_want / b->w_names, which are on the device (uploaded below, or the plan's); win[] starts all zero.  *cap = slots of the table
static int fx_want_table(mahip_ctx *c, UseqBufs *b, const char *who, size_t n_wanted, uint32_t *cap_out)
{
	if (n_wanted >= 0x40000000ull) { mahip_set_error("%s: too many wanted reads", who); return -1; }
	uint32_t cap = 64; while (cap < 2 * n_wanted) cap <<= 1;
	CHK(dev_reserve(c, b->fx_whash, (n_wanted ? n_wanted : 1) * 8));
	CHK(dev_reserve(c, b->fx_tab, (size_t)cap * 4)); CHK(dev_reserve(c, b->fx_win, (n_wanted ? n_wanted : 1) * 4));
	HIPCHK(hipMemsetAsync(b->fx_tab.p, 0, (size_t)cap * 4, c->st));
	if (n_wanted) HIPCHK(hipMemsetAsync(b->fx_win.p, 0, n_wanted * 4, c->st));
	if (n_wanted) {
		ProfScope ps(c, "k_fx_tab_build", 0);
		hipLaunchKernelGGL(k_fx_tab_build, dim3(grid_for(n_wanted, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, b->w_want, b->w_names, (uint32_t)n_wanted,
		                   P<uint64_t>(b->fx_whash), P<uint32_t>(b->fx_tab), cap - 1);
		HIPCHK(hipGetLastError());
	}
	*cap_out = cap;
	return 0;
}
// the wanted reads and their names from host memory to the device (once per file, once per stream), then the table
static int fx_want_upload(mahip_ctx *c, UseqBufs *b, const char *who, const mahip_useq_want_t *wanted, size_t n_wanted, const char *names, size_t name_bytes, uint32_t *cap_out)
{
	if (n_wanted >= 0x40000000ull) { mahip_set_error("%s: too many wanted reads", who); return -1; }
	for (size_t w = 0; w < n_wanted; ++w) // the kernels trust these
		if (wanted[w].name_off + wanted[w].name_len > name_bytes || wanted[w].dst_off + wanted[w].len > b->arena_bytes || (!wanted[w].whole && wanted[w].s > wanted[w].e)) {
			mahip_set_error("%s: wanted read %zu reaches outside the names or the arena", who, w); return -1;
		}
	CHK(dev_reserve(c, b->fx_want, (n_wanted ? n_wanted : 1) * sizeof(mahip_useq_want_t))); CHK(dev_reserve(c, b->fx_wname, name_bytes + 64));
	if (n_wanted) HIPCHK(hipMemcpyAsync(b->fx_want.p, wanted, n_wanted * sizeof(mahip_useq_want_t), hipMemcpyHostToDevice, c->st));
	if (name_bytes) HIPCHK(hipMemcpyAsync(b->fx_wname.p, names, name_bytes, hipMemcpyHostToDevice, c->st));
	b->w_want = (const mahip_useq_want_t*)b->fx_want.p; b->w_names = (const unsigned char*)b->fx_wname.p;
	return fx_want_table(c, b, who, n_wanted, cap_out);
}
static int pl_want_planned(mahip_ctx *c, UseqBufs *b, const char *who, size_t *n_wanted, uint32_t *cap_out); // the plan's table in their place (third part of this file)

static int fx_place_wanted(mahip_ctx *c, UseqBufs *b, size_t n_wanted, uint32_t cap, double t0, uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms);
extern "C" int mahip_useq_place_text(mahip_ctx_t *c, const mahip_useq_want_t *wanted, size_t n_wanted, const char *names, size_t name_bytes,
                                     uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fx_regular) { mahip_set_error("mahip_useq_place_text: no text in the regular form (mahip_fastx_index)"); return -1; }
	if (n_wanted >= 0x40000000ull) { mahip_set_error("mahip_useq_place_text: too many wanted reads"); return -1; }
	*n_matched = *n_dup = *n_short = 0;
	if (laps_ms) laps_ms[0] = laps_ms[1] = 0;
	if (n_wanted == 0 || b->fx_R == 0) return 0;
	const double t0 = fx_now();
	uint32_t cap = 0;
	CHK(fx_want_upload(c, b, "mahip_useq_place_text", wanted, n_wanted, names, name_bytes, &cap));
	return fx_place_wanted(c, b, n_wanted, cap, t0, n_matched, n_dup, n_short, laps_ms);
}
extern "C" int mahip_useq_place_text_planned(mahip_ctx_t *c, uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fx_regular) { mahip_set_error("mahip_useq_place_text_planned: no text in the regular form (mahip_fastx_index)"); return -1; }
	*n_matched = *n_dup = *n_short = 0;
	if (laps_ms) laps_ms[0] = laps_ms[1] = 0;
	const double t0 = fx_now();
	size_t n_wanted = 0;
	uint32_t cap = 0;
	CHK(pl_want_planned(c, b, "mahip_useq_place_text_planned", &n_wanted, &cap));
	if (n_wanted == 0 || b->fx_R == 0) return 0;
	return fx_place_wanted(c, b, n_wanted, cap, t0, n_matched, n_dup, n_short, laps_ms);
}
// everything behind the table: lookup, the SHORT_READ verdict, placement
static int fx_place_wanted(mahip_ctx *c, UseqBufs *b, size_t n_wanted, uint32_t cap, double t0, uint64_t *n_matched, uint64_t *n_dup, uint64_t *n_short, double *laps_ms)
{
	HIPCHK(hipMemsetAsync(b->fx_ctr.p, 0, FX_NCTR * 8, c->st));
	const FxText x = fx_view(b);
	{
		ProfScope ps(c, "k_fx_probe", 0);
		hipLaunchKernelGGL(k_fx_probe, dim3(grid_for(b->fx_R, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, x, b->w_want, b->w_names, (const uint64_t*)b->fx_whash.p,
		                   (const uint32_t*)b->fx_tab.p, cap - 1, P<uint32_t>(b->fx_win), P<unsigned long long>(b->fx_ctr));
		HIPCHK(hipGetLastError());
	}
	unsigned long long h[FX_NCTR];
	CHK(fx_counters(c, b, h)); // (waits for the uploads too: the caller may reuse wanted / names)
	*n_matched = h[FX_DISTINCT]; *n_dup = h[FX_MATCH] - h[FX_DISTINCT]; *n_short = h[FX_SHORT];
	const double t1 = fx_now();
	if (laps_ms) laps_ms[0] = (t1 - t0) * 1e3;
	if (h[FX_SHORT]) return 0; // the caller falls back: nothing has touched the arena
	{
		ProfScope ps(c, "k_fx_place", 0);
		hipLaunchKernelGGL(k_fx_place, dim3(grid_for(n_wanted, 1, 65536)), dim3(256), 0, c->st, x, b->w_want, (uint32_t)n_wanted, (const uint32_t*)b->fx_win.p, (unsigned char*)b->arena.p);
		HIPCHK(hipGetLastError());
	}
	if (laps_ms) { HIPCHK(hipStreamSynchronize(c->st)); laps_ms[1] = (fx_now() - t1) * 1e3; }
	return 0;
}

// ------------------------------------------------------------------------------------------------ the streamed reader (include/mahip.h)
static int fxw_begin(mahip_ctx *c, UseqBufs *b, size_t n_wanted, uint32_t cap);
extern "C" int mahip_useq_stream_begin(mahip_ctx_t *c, const mahip_useq_want_t *wanted, size_t n_wanted, const char *names, size_t name_bytes)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	b->fx_loaded = b->fx_regular = false; // the window takes the text buffer
	b->fw_active = false;
	uint32_t cap = 0;
	CHK(fx_want_upload(c, b, "mahip_useq_stream_begin", wanted, n_wanted, names, name_bytes, &cap));
	return fxw_begin(c, b, n_wanted, cap);
}
extern "C" int mahip_useq_stream_begin_planned(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	b->fx_loaded = b->fx_regular = false;
	b->fw_active = false;
	size_t n_wanted = 0;
	uint32_t cap = 0;
	CHK(pl_want_planned(c, b, "mahip_useq_stream_begin_planned", &n_wanted, &cap));
	return fxw_begin(c, b, n_wanted, cap);
}
// a stream over the table that is in place: the names seen so far, the window's state
static int fxw_begin(mahip_ctx *c, UseqBufs *b, size_t n_wanted, uint32_t cap)
{
	CHK(dev_reserve(c, b->fw_ctr, FXW_NCTR * 8)); CHK(dev_reserve(c, b->fw_seen, n_wanted ? n_wanted : 1));
	HIPCHK(hipMemsetAsync(b->fw_seen.p, 0, n_wanted ? n_wanted : 1, c->st));
	HIPCHK(hipStreamSynchronize(c->st)); // the caller may reuse wanted / names
	b->fw_mask = cap - 1; b->fw_n_want = n_wanted; b->fw_n = b->fw_carry_off = b->fw_carry = b->fw_cap = 0; b->fw_t_place = 0; // (the first piece brings the window's first buffer)
	memset(&b->fw_rep, 0, sizeof(b->fw_rep));
	b->fw_rep.refused_piece = -1;
	b->fw_active = true; b->fw_ended = false;
	return 0;
}

static int fxw_counters(mahip_ctx *c, UseqBufs *b, unsigned long long *h)
{
	HIPCHK(hipMemcpyAsync(h, b->fw_ctr.p, FXW_NCTR * 8, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	return 0;
}
// what is still running of the window before (its placement) ends here: the lap belongs to `place`
static int fxw_drain(mahip_ctx *c, UseqBufs *b)
{
	const double t0 = fx_now();
	HIPCHK(hipStreamSynchronize(c->st));
	b->fw_t_place += fx_now() - t0;
	b->fw_rep.laps_ms[3] = b->fw_t_place * 1e3;
	return 0;
}

#define FXW_RESERVE(buf, bytes) do { if (dev_reserve(c, (buf), (bytes)) != 0) { reason = MAHIP_FASTX_NOMEM; goto refuse; } } while (0)
extern "C" int mahip_useq_stream_piece_mem(mahip_ctx_t *c, const void *text, size_t nbytes, int last, mahip_useq_stream_verdict_t *v)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	mahip_useq_stream_report_t *rep = &b->fw_rep;
	memset(v, 0, sizeof(*v));
	if (!b->fw_active) { mahip_set_error("mahip_useq_stream_piece_mem: no stream (mahip_useq_stream_begin)"); return -1; }
	if (rep->refused_piece >= 0) { mahip_set_error("mahip_useq_stream_piece_mem: piece %lld was refused, the stream takes no more", (long long)rep->refused_piece); return -1; }
	if (b->fw_ended) { mahip_set_error("mahip_useq_stream_piece_mem: a piece behind the last one"); return -1; }
	if (!last && nbytes && ((const char*)text)[nbytes - 1] != '\n') { mahip_set_error("mahip_useq_stream_piece_mem: a piece that is not the last ends inside a line"); return -1; }
	const int64_t piece_no = (int64_t)rep->n_pieces++;
	if (last) b->fw_ended = true;
	double t0 = fx_now(), t1;
	int reason = MAHIP_FASTX_OK;
	unsigned long long h[FXW_NCTR];
	memset(h, 0, sizeof(h));
	// ---- the window: the carry to the front, the piece behind it
	CHK(fxw_drain(c, b)); // the placement of the window before reads the text
	t0 = fx_now();
	const size_t carry = b->fw_carry, n = carry + nbytes;
	if (n + 64 > b->fw_cap) { // a record longer than the window: a larger one, by half as much again as is needed now (fw_cap: what was asked for -- the pool may have given more)
		DevBuf nw;
		CHK(dev_reserve(c, nw, n + n / 2 + 64)); // (no room for ONE record and a piece: an error, not a verdict -- the window could not be handed back whole)
		if (carry) HIPCHK(hipMemcpyAsync(nw.p, (const char*)b->fx_text.p + b->fw_carry_off, carry, hipMemcpyDeviceToDevice, c->st));
		HIPCHK(hipStreamSynchronize(c->st));
		if (b->fw_cap) ++rep->n_window_grow;
		dev_free(c, b->fx_text);
		b->fx_text = nw; b->fw_cap = n + n / 2 + 64;
	} else if (carry && b->fw_carry_off) {
		if (carry <= b->fw_carry_off) HIPCHK(hipMemcpyAsync(b->fx_text.p, (const char*)b->fx_text.p + b->fw_carry_off, carry, hipMemcpyDeviceToDevice, c->st));
		else {
			hipLaunchKernelGGL(k_fxw_move, dim3(1), dim3(256), 0, c->st, (unsigned char*)b->fx_text.p, (uint64_t)b->fw_carry_off, (uint64_t)carry);
			HIPCHK(hipGetLastError());
		}
	}
	b->fw_carry_off = 0; b->fw_n = n;
	if (nbytes) CHK(xfer_copy(c, (char*)b->fx_text.p + carry, (void*)text, nbytes, 1));
	else HIPCHK(hipStreamSynchronize(c->st));
	rep->laps_ms[0] += ((t1 = fx_now()) - t0) * 1e3; t0 = t1;
	if (n == 0) return 0; // nothing yet, or nothing at all
	if (rep->format == 0) { // the first byte of the INPUT fixes the format of every window (window 0 holds no carry)
		const unsigned char c0 = *(const unsigned char*)text;
		rep->format = c0 == '>' ? MAHIP_FASTX_FASTA : c0 == '@' ? MAHIP_FASTX_FASTQ : 0;
		if (rep->format == 0) { reason = MAHIP_FASTX_FIRST_BYTE; goto refuse; }
	}
	{
		// ---- the line index of the window (the whole-file reader's census and line starts)
		if ((n + FX_GRAN - 1) / FX_GRAN > 0xffffffffull) { reason = MAHIP_FASTX_TOO_MANY_LINES; goto refuse; }
		const uint32_t n_gran = (uint32_t)((n + FX_GRAN - 1) / FX_GRAN);
		const bool fq = rep->format == MAHIP_FASTX_FASTQ;
		unsigned long long *ctr = P<unsigned long long>(b->fw_ctr);
		FXW_RESERVE(b->fx_gcnt, (size_t)n_gran * 4); FXW_RESERVE(b->fx_gpos, (size_t)n_gran * 4 + 4);
		HIPCHK(hipMemsetAsync(ctr, 0, FXW_NCTR * 8, c->st));
		{
			ProfScope ps(c, "k_fx_census", (double)n);
			hipLaunchKernelGGL(k_fx_census, dim3(grid_for(n_gran, 4, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const unsigned char*)b->fx_text.p, (uint64_t)n, n_gran, P<uint32_t>(b->fx_gcnt), ctr);
			HIPCHK(hipGetLastError());
		}
		CHK(fxw_counters(c, b, h));
		const uint64_t L = h[FX_NL] + (h[FX_LAST] != '\n');
		if (L > 0xffffffffull) { reason = MAHIP_FASTX_TOO_MANY_LINES; goto refuse; }
		const size_t list_cap = (L < b->fw_n_want ? (size_t)L : b->fw_n_want) + 1; // a wanted read enters the list once a window, a record once
		FXW_RESERVE(b->fx_ls, (size_t)(L + 2) * 8); FXW_RESERVE(b->fw_list, list_cap * 4);
		if (!fq) { FXW_RESERVE(b->fx_hdr, (size_t)L * 4); FXW_RESERVE(b->fx_hpos, (size_t)(L + 1) * 4); FXW_RESERVE(b->fx_recl, (size_t)(L + 1) * 4); }
		CHK(scan_exclusive_u32(c, P<uint32_t>(b->fx_gcnt), P<uint32_t>(b->fx_gpos), n_gran, nullptr));
		{
			ProfScope ps(c, "k_fx_lines", (double)n + 8.0 * (double)L);
			hipLaunchKernelGGL(k_fx_lines, dim3(grid_for(n_gran, 4, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const unsigned char*)b->fx_text.p, (uint64_t)n, n_gran, P<uint32_t>(b->fx_gpos), (uint32_t)L, P<uint64_t>(b->fx_ls));
			HIPCHK(hipGetLastError());
		}
		// ---- the consumed prefix, its records, its form: L and R of the prefix stay on the device
		const FxText x = {(const unsigned char*)b->fx_text.p, (const uint64_t*)b->fx_ls.p, (const uint32_t*)b->fx_recl.p, (uint64_t)n, (uint32_t)L, 0u, fq};
		const unsigned g_lines = grid_for(L, 256, MA_STREAM_BLOCKS);
		ProfScope ps(c, "k_fxw_window", (double)n);
		if (!fq) {
			hipLaunchKernelGGL(k_fxw_hdr, dim3(g_lines), dim3(256), 0, c->st, x, P<uint32_t>(b->fx_hdr), ctr);
			HIPCHK(hipGetLastError());
			CHK(scan_exclusive_u32(c, P<uint32_t>(b->fx_hdr), P<uint32_t>(b->fx_hpos), L, P<uint32_t>(b->fx_hpos) + L));
		}
		hipLaunchKernelGGL(k_fxw_prefix, dim3(1), dim3(64), 0, c->st, x, (const uint32_t*)b->fx_hpos.p, last ? 1 : 0, ctr);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_fxw_bytes, dim3(grid_for(n_gran, 4, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const unsigned char*)b->fx_text.p, ctr);
		HIPCHK(hipGetLastError());
		if (!fq) {
			hipLaunchKernelGGL(k_fxw_rec_lines, dim3(g_lines), dim3(256), 0, c->st, (const uint32_t*)b->fx_hdr.p, (const uint32_t*)b->fx_hpos.p, (const unsigned long long*)ctr, P<uint32_t>(b->fx_recl));
			HIPCHK(hipGetLastError());
			hipLaunchKernelGGL(k_fxw_form_fasta, dim3(g_lines), dim3(256), 0, c->st, x, P<uint32_t>(b->fx_hdr), ctr);
		} else hipLaunchKernelGGL(k_fxw_form_fastq, dim3(grid_for(L / 4, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, x, ctr);
		HIPCHK(hipGetLastError());
		rep->laps_ms[1] += ((t1 = fx_now()) - t0) * 1e3; t0 = t1;
		// ---- the names of the prefix's records against the table; the wanted reads that matched go to the list
		hipLaunchKernelGGL(k_fxw_probe, dim3(grid_for(fq ? L / 4 : L, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, x, b->w_want, b->w_names,
		                   (const uint64_t*)b->fx_whash.p, (const uint32_t*)b->fx_tab.p, b->fw_mask, P<uint32_t>(b->fx_win), (const unsigned char*)b->fw_seen.p, P<uint32_t>(b->fw_list), ctr);
		HIPCHK(hipGetLastError());
		CHK(fxw_counters(c, b, h));
		rep->laps_ms[2] += ((t1 = fx_now()) - t0) * 1e3; t0 = t1;
		// ---- the verdict, before the arena is touched (the whole-file reader's order of reasons)
		if (h[FXW_CR]) reason = MAHIP_FASTX_CR;
		else if (h[FXW_NUL]) reason = MAHIP_FASTX_NUL_BYTE;
		else if (fq && last && L % 4) reason = MAHIP_FASTX_FASTQ_SHAPE;
		else if (h[FX_V_FASTA]) reason = MAHIP_FASTX_FASTA_LINE_START;
		else if (h[FX_V_SHAPE]) reason = MAHIP_FASTX_FASTQ_SHAPE;
		else if (h[FX_V_QUAL]) reason = MAHIP_FASTX_FASTQ_QUAL_LEN;
		else if (h[FX_V_LONG]) reason = MAHIP_FASTX_LONG_LINE;
		else if (h[FX_SHORT]) reason = MAHIP_FASTX_SHORT_READ;
		if (reason != MAHIP_FASTX_OK) goto refuse;
		if (h[FXW_NLIST] >= list_cap) { mahip_set_error("mahip_useq_stream_piece_mem: the match list overflowed"); return -1; } // (cannot happen: see list_cap)
		if (h[FXW_NLIST]) {
			ProfScope pp(c, "k_fxw_place", 0);
			hipLaunchKernelGGL(k_fxw_place, dim3(grid_for(h[FXW_NLIST], 1, 65536)), dim3(256), 0, c->st, x, b->w_want, (const uint32_t*)b->fw_list.p, (uint32_t)h[FXW_NLIST],
			                   P<uint32_t>(b->fx_win), P<unsigned char>(b->fw_seen), (unsigned char*)b->arena.p);
			HIPCHK(hipGetLastError());
		}
		b->fw_t_place += fx_now() - t0; rep->laps_ms[3] = b->fw_t_place * 1e3;
		b->fw_carry_off = (size_t)h[FXW_CONSUMED]; b->fw_carry = (size_t)h[FXW_CARRY];
		v->n_records = h[FXW_R]; v->bytes_consumed = h[FXW_CONSUMED]; v->carry_bytes = h[FXW_CARRY]; v->n_placed = h[FXW_NLIST];
		rep->n_records += h[FXW_R]; rep->n_matched += h[FX_DISTINCT]; rep->n_dup += h[FX_MATCH] - h[FX_DISTINCT]; rep->n_jobs += h[FXW_NLIST];
		if (h[FXW_CARRY] > rep->max_carry) rep->max_carry = h[FXW_CARRY];
		return 0;
	}
refuse: // not an error: the window stays where it is (mahip_useq_stream_window_download), nothing of it has reached the arena
	v->reason = reason; v->n_records = h[FXW_R]; v->carry_bytes = h[FXW_CARRY]; v->bytes_consumed = 0; v->n_placed = 0;
	rep->refused_piece = piece_no; rep->refused_reason = reason; rep->n_short += h[FX_SHORT];
	return 0;
}
#undef FXW_RESERVE

extern "C" int mahip_useq_stream_window_download(mahip_ctx_t *c, void *dst, uint64_t *nbytes)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fw_active || b->fw_rep.refused_piece < 0) { mahip_set_error("mahip_useq_stream_window_download: no refused window"); return -1; }
	*nbytes = b->fw_n;
	if (dst && b->fw_n) CHK(xfer_copy(c, b->fx_text.p, dst, b->fw_n, 0));
	return 0;
}
extern "C" int mahip_useq_stream_end(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	if (!b->fw_active) { mahip_set_error("mahip_useq_stream_end: no stream"); return -1; }
	CHK(fxw_drain(c, b));
	b->fw_active = false;
	return 0;
}
extern "C" int mahip_useq_stream_abort(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	if (c->useq) { HIPCHK(hipStreamSynchronize(c->st)); ((UseqBufs*)c->useq)->fw_active = false; }
	return 0;
}
extern "C" int mahip_useq_stream_last(mahip_ctx_t *c, mahip_useq_stream_report_t *out) { *out = useq_bufs(c)->fw_rep; return 0; }

// ================================================================================================ the placement plan on the device (include/mahip.h)
// asm.c:248-260 and host/unitig_gfa.c: ug_seq_wanted over arrays that lie in HBM already: unitigs (u_len, first member, member words), names (blob, off), kept
// intervals.  Index work only:
//   uoff    exclusive scan of u_len[i] + 1 in 64 bits: one tile of 2048 values per block -- every thread sums 8, a wave scan over the thread sums (both halves of the
//           word travel through the cross-lane shifts together), the four wave totals through LDS.  More than one tile: the tile sums first, ONE block scans them
//           in place (256 at a time, carrying the running total), then every tile scans its values on top of its base
//   start   tc_ug_member_start over the scan of the members' low words (text_dev.hpp: text_ug_member_scan), as the `a` lines
//   scatter one thread per member: its unitig by bisection over the first-member array, its read's counter up by one (vector atomic); the first member to arrive
//           writes the read's place, any other is counted: MULTI
//   wanted  a flag per read (len != 0 and a name), scan_exclusive_u32, one table entry per flagged read at its scanned position: ascending read id
// The table's names stay where mahip_text_names put them: name_off is the read's offset in THAT blob, and the lookup kernels read `names + name_off` whichever
// blob `names` is (k_fx_tab_build, fx_lookup).
#define PL_ITEMS 8u
#define PL_TILE (256u * PL_ITEMS)
enum { PL_TOT = 0, PL_MULTI, PL_BAD, PL_NAMEB, PL_OOB, PL_NCTR = 8 };

__device__ __forceinline__ uint64_t wv_scan_incl_u64(uint64_t x, unsigned lane)
{
	for (int o = 1; o < 64; o <<= 1) { // (every lane of the wave is here)
		const uint32_t lo = __shfl_up((uint32_t)x, o, 64), hi = __shfl_up((uint32_t)(x >> 32), o, 64);
		if (lane >= (unsigned)o) x += (uint64_t)hi << 32 | lo;
	}
	return x;
}
// block-wide exclusive scan of one u64 per thread (256 threads); s_wave: 4 words of LDS
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t x, uint64_t *s_wave, uint64_t *total)
{
	const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t incl = wv_scan_incl_u64(x, lane);
	if (lane == 63) s_wave[wave] = incl;
	__syncthreads();
	uint64_t base = 0, tot = 0;
	for (unsigned w = 0; w < 4; ++w) { const uint64_t v = s_wave[w]; if (w < wave) base += v; tot += v; }
	__syncthreads();
	*total = tot;
	return base + incl - x;
}
// the 8 values of this thread in tile blockIdx.x: u_len[i] + 1, 0 behind the end; returns their sum
__device__ __forceinline__ uint64_t pl_tile_load(const uint32_t *__restrict__ u_len, uint32_t U, uint64_t v[PL_ITEMS])
{
	const uint64_t base = (uint64_t)blockIdx.x * PL_TILE + threadIdx.x * PL_ITEMS;
	uint64_t s = 0;
	for (uint32_t k = 0; k < PL_ITEMS; ++k) { v[k] = base + k < U ? (uint64_t)u_len[base + k] + 1u : 0u; s += v[k]; }
	return s;
}
__global__ __launch_bounds__(256) void k_pl_uoff_sums(const uint32_t *__restrict__ u_len, uint32_t U, uint64_t *__restrict__ bsum)
{
	__shared__ uint64_t s_wave[4];
	uint64_t v[PL_ITEMS], tot;
	block_excl_scan_u64(pl_tile_load(u_len, U, v), s_wave, &tot);
	if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_pl_uoff_bases(uint64_t *__restrict__ bsum, uint32_t nb) // one block, in place
{
	__shared__ uint64_t s_wave[4];
	uint64_t run = 0;
	for (uint32_t b0 = 0; b0 < nb; b0 += 256) { // (the whole block)
		const uint32_t i = b0 + threadIdx.x;
		const uint64_t x = i < nb ? bsum[i] : 0;
		uint64_t tot;
		const uint64_t ex = block_excl_scan_u64(x, s_wave, &tot);
		if (i < nb) bsum[i] = run + ex;
		run += tot;
	}
}
// uoff[i] for the tile's unitigs; the thread that holds the last unitig also writes uoff[U] = ctr[PL_TOT] = the arena's bytes.  bbase == 0: a single tile
__global__ __launch_bounds__(256) void k_pl_uoff_down(const uint32_t *__restrict__ u_len, uint32_t U, const uint64_t *__restrict__ bbase, uint64_t *__restrict__ uoff, unsigned long long *__restrict__ ctr)
{
	__shared__ uint64_t s_wave[4];
	uint64_t v[PL_ITEMS], tot;
	const uint64_t base = (uint64_t)blockIdx.x * PL_TILE + threadIdx.x * PL_ITEMS;
	uint64_t run = block_excl_scan_u64(pl_tile_load(u_len, U, v), s_wave, &tot) + (bbase ? bbase[blockIdx.x] : 0);
	for (uint32_t k = 0; k < PL_ITEMS; ++k) {
		if (base + k < U) uoff[base + k] = run;
		run += v[k];
		if (base + k + 1 == U) { uoff[U] = run; ctr[PL_TOT] = run; }
	}
}
// cnt[read] += 1 per member; place[read] = (utg, start, len, ori) by the member that came first
__global__ __launch_bounds__(256) void k_pl_scatter(const uint64_t *__restrict__ mem, uint32_t M, const uint32_t *__restrict__ moff, uint32_t U, const uint32_t *__restrict__ mscan, uint32_t n_reads,
                                                    uint32_t *__restrict__ cnt, uint4 *__restrict__ place, unsigned long long *__restrict__ ctr)
{
	uint64_t multi = 0, bad = 0;
	for (uint64_t m = (uint64_t)blockIdx.x * 256u + threadIdx.x; m < M; m += (uint64_t)gridDim.x * 256u) {
		const uint64_t w = mem[m];
		const uint32_t read = (uint32_t)(w >> 33);
		uint32_t lo = 0, hi = U; // the last unitig whose first member is not behind m (a unitig without members shares its successor's first member and lies in front of it)
		while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (moff[mid] <= m) lo = mid; else hi = mid; }
		if (read >= n_reads) { ++bad; continue; }
		if (atomicAdd(&cnt[read], 1u) != 0u) { ++multi; continue; } // asm.c:255 asserts here
		place[read] = make_uint4(lo, tc_ug_member_start(mscan, moff[lo], (uint32_t)m), (uint32_t)w, (uint32_t)(w >> 32) & 1u); // asm.c:254-258
	}
	blk_add_u64(ctr + PL_MULTI, multi);
	blk_add_u64(ctr + PL_BAD, bad);
}
// flag[r] = read r is wanted: it sits on a unitig with len != 0 and has a name (host/unitig_gfa.c: ug_seq_wanted); ctr[PL_NAMEB] += the bytes of their names
__global__ __launch_bounds__(256) void k_pl_flag(const uint4 *__restrict__ place, const uint64_t *__restrict__ off, uint32_t n_reads, uint32_t *__restrict__ flag, unsigned long long *__restrict__ ctr)
{
	uint64_t nb = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * 256u) {
		const uint64_t l = off[r + 1] - off[r];
		const uint32_t f = place[r].z != 0u && l != 0u;
		flag[r] = f;
		if (f) nb += l;
	}
	blk_add_u64(ctr + PL_NAMEB, nb);
}
// the table entry of every wanted read at its scanned position; ctr[PL_OOB] += entries that reach outside the arena or whose interval is upside down (the planned
// readers refuse such a plan: the placement trusts the table).  sub: word 2 r = s | del << 31, word 2 r + 1 = e; 0: whole records
__global__ __launch_bounds__(256) void k_pl_want(const uint4 *__restrict__ place, const uint64_t *__restrict__ off, const uint64_t *__restrict__ uoff, const uint32_t *__restrict__ sub,
                                                 const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint32_t n_reads, uint32_t U, mahip_useq_want_t *__restrict__ want,
                                                 unsigned long long *__restrict__ ctr)
{
	const uint64_t tot = uoff[U];
	uint64_t oob = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * 256u) {
		if (!flag[r]) continue;
		const uint4 p = place[r];
		mahip_useq_want_t w;
		w.dst_off = uoff[p.x] + p.y; w.name_off = off[r]; w.name_len = (uint32_t)(off[r + 1] - off[r]);
		w.len = p.z; w.s = sub ? sub[2 * r] & 0x7fffffffu : 0u; w.e = sub ? sub[2 * r + 1] : 0u; w.rev = p.w; w.whole = sub == nullptr;
		oob += w.dst_off + w.len > tot || w.s > w.e;
		want[pos[r]] = w;
	}
	blk_add_u64(ctr + PL_OOB, oob);
}

extern "C" const char *mahip_useq_plan_reason_name(int reason)
{
	static const char *const nm[] = {"ok", "no unitigs on the device", "the names are not on the device", "a read sits on a unitig more than once", "no device memory for the plan", "MA_USEQ_PLAN_HOST is set"};
	return reason >= 0 && reason < (int)(sizeof(nm) / sizeof(nm[0])) ? nm[reason] : "?";
}
void useq_plan_drop(mahip_ctx *c) { if (c->useq) ((UseqBufs*)c->useq)->pl_valid = false; }
static bool pl_forced() { const char *e = getenv("MA_USEQ_PLAN_HOST"); return e && atoi(e) != 0; }
static int pl_refuse(UseqBufs *b, mahip_useq_plan_info_t *info, int reason, double t0)
{
	info->road = MAHIP_PLAN_ROAD_HOST; info->reason = reason; info->ms = (fx_now() - t0) * 1e3;
	b->pl_valid = false; b->pl_info = *info;
	return 0;
}

struct PlanSrc { uint32_t U, M, n_reads; const uint32_t *u_len, *moff; const uint64_t *mem; const unsigned char *blob; const uint64_t *off; uint64_t blob_bytes, names_gen; const uint32_t *sub; bool ctx; };

// the plan itself: everything is queued, the host waits once (for the counters)
static int pl_run(mahip_ctx *c, UseqBufs *b, const PlanSrc &s, mahip_useq_plan_info_t *info, double t0)
{
	const uint32_t U = s.U, M = s.M, R = s.n_reads, nb = (U + PL_TILE - 1) / PL_TILE;
	const size_t most = M < R ? M : R; // wanted reads at the most
	info->n_utg = U; info->n_members = M; info->n_reads = R; info->blob_bytes = s.blob_bytes; info->uoff_tiles = nb;
	if (dev_reserve(c, b->pl_uoff, ((size_t)U + 2) * 8) != 0 || dev_reserve(c, b->pl_bsum, ((size_t)nb + 2) * 8) != 0 || dev_reserve(c, b->pl_low, ((size_t)M + 16) * 4) != 0 ||
	    dev_reserve(c, b->pl_mscan, ((size_t)M + 16) * 4) != 0 || dev_reserve(c, b->pl_cnt, ((size_t)R + 16) * 4) != 0 || dev_reserve(c, b->pl_place, ((size_t)R + 1) * 16) != 0 ||
	    dev_reserve(c, b->pl_flag, ((size_t)R + 16) * 4) != 0 || dev_reserve(c, b->pl_pos, ((size_t)R + 16) * 4) != 0 || dev_reserve(c, b->pl_want, (most + 1) * sizeof(mahip_useq_want_t)) != 0 ||
	    dev_reserve(c, b->pl_ctr, PL_NCTR * 8) != 0)
		return pl_refuse(b, info, MAHIP_PLAN_NOMEM, t0);
	unsigned long long *ctr = P<unsigned long long>(b->pl_ctr);
	uint4 *place = (uint4*)b->pl_place.p;
	HIPCHK(hipMemsetAsync(ctr, 0, PL_NCTR * 8, c->st));
	HIPCHK(hipMemsetAsync(b->pl_cnt.p, 0, ((size_t)R + 16) * 4, c->st));
	HIPCHK(hipMemsetAsync(place, 0, ((size_t)R + 1) * 16, c->st)); // a read on no unitig: len 0
	{
		ProfScope ps(c, "k_pl_uoff", 12.0 * (double)U);
		if (nb > 1) {
			hipLaunchKernelGGL(k_pl_uoff_sums, dim3(nb), dim3(256), 0, c->st, s.u_len, U, P<uint64_t>(b->pl_bsum));
			hipLaunchKernelGGL(k_pl_uoff_bases, dim3(1), dim3(256), 0, c->st, P<uint64_t>(b->pl_bsum), nb);
		}
		hipLaunchKernelGGL(k_pl_uoff_down, dim3(nb), dim3(256), 0, c->st, s.u_len, U, nb > 1 ? (const uint64_t*)b->pl_bsum.p : (const uint64_t*)nullptr, P<uint64_t>(b->pl_uoff), ctr);
		HIPCHK(hipGetLastError());
	}
	CHK(text_ug_member_scan(c, s.mem, M, P<uint32_t>(b->pl_low), P<uint32_t>(b->pl_mscan)));
	{
		ProfScope ps(c, "k_pl_scatter", 28.0 * (double)M);
		hipLaunchKernelGGL(k_pl_scatter, dim3(grid_for(M, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, s.mem, M, s.moff, U, (const uint32_t*)b->pl_mscan.p, R, P<uint32_t>(b->pl_cnt), place, ctr);
		HIPCHK(hipGetLastError());
	}
	{
		ProfScope ps(c, "k_pl_flag", 28.0 * (double)R);
		hipLaunchKernelGGL(k_pl_flag, dim3(grid_for(R, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const uint4*)place, s.off, R, P<uint32_t>(b->pl_flag), ctr);
		HIPCHK(hipGetLastError());
	}
	CHK(scan_exclusive_u32(c, P<uint32_t>(b->pl_flag), P<uint32_t>(b->pl_pos), R, P<uint32_t>(b->pl_pos) + R));
	{
		ProfScope ps(c, "k_pl_want", 40.0 * (double)R);
		hipLaunchKernelGGL(k_pl_want, dim3(grid_for(R, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, (const uint4*)place, s.off, (const uint64_t*)b->pl_uoff.p, s.sub, (const uint32_t*)b->pl_flag.p,
		                   (const uint32_t*)b->pl_pos.p, R, U, (mahip_useq_want_t*)b->pl_want.p, ctr);
		HIPCHK(hipGetLastError());
	}
	unsigned long long h[PL_NCTR];
	uint32_t n_want = 0;
	HIPCHK(hipMemcpyAsync(h, ctr, PL_NCTR * 8, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipMemcpyAsync(&n_want, P<uint32_t>(b->pl_pos) + R, 4, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	info->n_multi = h[PL_MULTI]; info->arena_bytes = h[PL_TOT];
	if (h[PL_BAD]) { b->pl_valid = false; mahip_set_error("mahip_useq_plan: %llu members name a read outside the %u reads of the names", h[PL_BAD], R); return -1; }
	if (h[PL_MULTI]) return pl_refuse(b, info, MAHIP_PLAN_MULTI, t0);
	info->n_wanted = n_want; info->name_bytes = h[PL_NAMEB];
	info->road = MAHIP_PLAN_ROAD_DEVICE; info->reason = MAHIP_PLAN_OK; info->ms = (fx_now() - t0) * 1e3;
	b->pl_valid = true; b->pl_ctx = s.ctx; b->pl_names_gen = s.names_gen; b->pl_bad = h[PL_OOB]; b->pl_blob = s.blob;
	b->pl_info = *info;
	return 0;
}

uint32_t graph_nseq(const mahip_ctx *c); // graph.hip

extern "C" int mahip_useq_plan(mahip_ctx_t *c, int have_sub, mahip_useq_plan_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	mahip_useq_plan_info_t tmp;
	if (!info) info = &tmp;
	memset(info, 0, sizeof(*info));
	const double t0 = fx_now();
	b->pl_valid = false;
	if (pl_forced()) return pl_refuse(b, info, MAHIP_PLAN_FORCED, t0);
	UgDevView v;
	if (!ug_dev_view(c, &v)) return pl_refuse(b, info, MAHIP_PLAN_NO_UG, t0);
	PlanSrc s = {v.U, v.M, graph_nseq(c), v.u_len, v.u_off, v.mem, nullptr, nullptr, 0, 0, nullptr, true};
	const char *blob = nullptr;
	uint32_t n_names = 0;
	if (!text_dev_names(c, &blob, &s.off, &n_names, &s.blob_bytes, &s.names_gen) || n_names != s.n_reads) return pl_refuse(b, info, MAHIP_PLAN_NO_NAMES, t0);
	s.blob = (const unsigned char*)blob;
	if (have_sub) { // slot 0, as mahip_sub_download hands it over
		const int rc = text_dev_sub(c, s.n_reads, &s.sub);
		if (rc < 0) return -1;
		if (rc > 0) return pl_refuse(b, info, MAHIP_PLAN_NOMEM, t0);
	}
	return pl_run(c, b, s, info, t0);
}

extern "C" int mahip_useq_plan_mem(mahip_ctx_t *c, uint32_t n_utg, const uint32_t *u_n, const uint32_t *u_len, const uint64_t *members, uint32_t n_seq, const char *blob, const uint64_t *off,
                                   const void *sub, mahip_useq_plan_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	mahip_useq_plan_info_t tmp;
	if (!info) info = &tmp;
	memset(info, 0, sizeof(*info));
	const double t0 = fx_now();
	b->pl_valid = false;
	if (pl_forced()) return pl_refuse(b, info, MAHIP_PLAN_FORCED, t0);
	if (n_utg == 0) return pl_refuse(b, info, MAHIP_PLAN_NO_UG, t0);
	if (!blob || !off) return pl_refuse(b, info, MAHIP_PLAN_NO_NAMES, t0);
	uint64_t M = 0;
	for (uint32_t i = 0; i < n_utg; ++i) M += u_n[i];
	if (M > 0xffffffffull) { mahip_set_error("mahip_useq_plan_mem: the members do not fit 32 bits"); return -1; }
	CHK(mahip_text_names(c, blob, off, n_seq, nullptr));
	struct { DevBuf *b; const void *src; size_t bytes; } up[] = {{&b->pl_un, u_n, (size_t)n_utg * 4}, {&b->pl_ulen, u_len, (size_t)n_utg * 4}, {&b->pl_mem, members, (size_t)M * 8}, {&b->pl_sub, sub, sub ? (size_t)n_seq * 8 : 0}};
	for (auto &u : up) {
		if (dev_reserve(c, *u.b, u.bytes + 16) != 0) return pl_refuse(b, info, MAHIP_PLAN_NOMEM, t0);
		if (u.bytes) CHK(xfer_copy(c, u.b->p, (void*)u.src, u.bytes, 1));
	}
	if (dev_reserve(c, b->pl_moff, ((size_t)n_utg + 16) * 4) != 0) return pl_refuse(b, info, MAHIP_PLAN_NOMEM, t0);
	CHK(scan_exclusive_u32(c, P<uint32_t>(b->pl_un), P<uint32_t>(b->pl_moff), n_utg, nullptr));
	PlanSrc s = {n_utg, (uint32_t)M, n_seq, P<uint32_t>(b->pl_ulen), P<uint32_t>(b->pl_moff), (const uint64_t*)b->pl_mem.p, nullptr, nullptr, 0, 0, sub ? P<uint32_t>(b->pl_sub) : nullptr, false};
	const char *d_blob = nullptr;
	uint32_t n_names = 0;
	if (!text_dev_names(c, &d_blob, &s.off, &n_names, &s.blob_bytes, &s.names_gen)) { mahip_set_error("mahip_useq_plan_mem: the names did not reach the device"); return -1; }
	s.blob = (const unsigned char*)d_blob;
	return pl_run(c, b, s, info, t0);
}

extern "C" int mahip_useq_plan_last(mahip_ctx_t *c, mahip_useq_plan_info_t *info) { *info = useq_bufs(c)->pl_info; return 0; }

// a plan is there, and the names its table points into are still the ones it was made of
static int pl_have(mahip_ctx *c, UseqBufs *b, const char *who)
{
	const char *blob; const uint64_t *off; uint32_t n; uint64_t bytes, gen = 0;
	if (!b->pl_valid) { mahip_set_error("%s: the context holds no placement plan (mahip_useq_plan)", who); return -1; }
	if (!text_dev_names(c, &blob, &off, &n, &bytes, &gen) || gen != b->pl_names_gen) { mahip_set_error("%s: the names the plan points into were replaced (mahip_text_names)", who); return -1; }
	return 0;
}
bool useq_plan_uoff(mahip_ctx *c, uint32_t U, uint32_t M, const uint64_t **d_uoff, uint64_t *tot)
{
	UseqBufs *b = (UseqBufs*)c->useq;
	if (!b || !b->pl_valid || !b->pl_ctx || b->pl_info.n_utg != U || b->pl_info.n_members != M) return false;
	*d_uoff = (const uint64_t*)b->pl_uoff.p; *tot = b->pl_info.arena_bytes;
	return true;
}

extern "C" int mahip_useq_plan_download(mahip_ctx_t *c, uint64_t *uoff, mahip_useq_place_t *pl, mahip_useq_want_t *want, char *names)
{
	HIPCHK(hipSetDevice(c->dev));
	UseqBufs *b = useq_bufs(c);
	CHK(pl_have(c, b, "mahip_useq_plan_download"));
	const mahip_useq_plan_info_t &pi = b->pl_info;
	if (uoff) HIPCHK(hipMemcpyAsync(uoff, b->pl_uoff.p, ((size_t)pi.n_utg + 1) * 8, hipMemcpyDeviceToHost, c->st));
	if (pl && pi.n_reads) HIPCHK(hipMemcpyAsync(pl, b->pl_place.p, (size_t)pi.n_reads * sizeof(mahip_useq_place_t), hipMemcpyDeviceToHost, c->st));
	if (want && pi.n_wanted) HIPCHK(hipMemcpyAsync(want, b->pl_want.p, (size_t)pi.n_wanted * sizeof(mahip_useq_want_t), hipMemcpyDeviceToHost, c->st));
	if (names && pi.blob_bytes) HIPCHK(hipMemcpyAsync(names, b->pl_blob, (size_t)pi.blob_bytes, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	return 0;
}

extern "C" int mahip_useq_begin_planned(mahip_ctx_t *c)
{
	UseqBufs *b = useq_bufs(c);
	CHK(pl_have(c, b, "mahip_useq_begin_planned"));
	return mahip_useq_begin(c, (size_t)b->pl_info.arena_bytes);
}
static int pl_want_planned(mahip_ctx *c, UseqBufs *b, const char *who, size_t *n_wanted, uint32_t *cap_out)
{
	CHK(pl_have(c, b, who));
	if (b->arena_bytes != b->pl_info.arena_bytes) { mahip_set_error("%s: the arena is not the plan's (mahip_useq_begin_planned)", who); return -1; }
	if (b->pl_bad) { mahip_set_error("%s: %llu entries of the plan's table reach outside the arena or hold an interval with s > e", who, (unsigned long long)b->pl_bad); return -1; } // (the kernels trust the table)
	b->w_want = (const mahip_useq_want_t*)b->pl_want.p; b->w_names = b->pl_blob;
	*n_wanted = (size_t)b->pl_info.n_wanted;
	return fx_want_table(c, b, who, *n_wanted, cap_out);
}

extern "C" void mahip_useq_note(mahip_ctx_t *c, const mahip_useq_info_t *in) { useq_bufs(c)->last = *in; }
extern "C" int mahip_useq_last(mahip_ctx_t *c, mahip_useq_info_t *out) { *out = useq_bufs(c)->last; return 0; }
