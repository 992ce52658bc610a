// paf.hip -- PAF text -> hit records + read-name dictionary on the device.
//
// Reproduces, bit for bit, what the reference's reader and ma_hit_read produce before the sort
// (paf.c:34-67 paf_parse/paf_read, kseq.h line semantics, sdict.c:27-45 sd_put, hit.c:70-101):
//   * a record is a line split on TABs; a trailing CR is dropped when the line is longer than one char;
//     lines with fewer than 10 columns are skipped; with exactly 10 columns `bl` keeps the value of the last
//     line that had an 11th column (0 before any);
//   * numeric columns follow strtol (leading blanks, sign, junk after the digits, saturation at LONG_MAX/MIN)
//     and are truncated to 32 bits (ml, bl to 31); rev = first char of column 5 is '-';
//   * a line is stored when both spans >= min_span and ml >= min_match (hit.c:85); its query name, then its target
//     name, enter the dictionary: ids are dense in order of FIRST APPEARANCE, the first length seen wins;
//   * every stored line yields the hit and, with bi_dir and qid != tid, the mirrored hit right after it.
// The sequential parts of the reference become data-parallel as follows: line starts = positions after '\n'
// (count, scan, scatter); first-appearance ids = hash-table insert with an atomic MIN of the occurrence number
// (2*line + column) per distinct name, then a sort of the distinct names by that minimum; the stale `bl` = a
// compaction of the lines that have one plus a prefix count; record slots = prefix sum of 1-or-2 per line.
// All HBM-bound byte/integer work: text is read once (through LDS tiles), per-line columns are 61 B.
#include "mahip_internal.hpp"
#include <time.h>

#define PAF_PROBE_LIMIT 2048u
#define PAF_EMPTY 0xffffffffffffffffull

// counter slots used by this file (aliases into ctx->ctr)
#define PC_VALID CT_LIVE
#define PC_PASS CT_REMAIN
#define PC_NOBL CT_OVF
#define PC_MAXQS CT_MAXQS
#define PC_OVERFLOW CT_OVF2
#define PC_DISTINCT CT_NMULTI

struct PafBufs {
	DevBuf text, lstart, tile;
	DevBuf glast, gmax, tfirst; // tile parser: last newline per granule / per group of granules, first line start per tile
	DevBuf flags, num[8], tnoff, qlen, tlen, hq, ht, qslot, tslot;
	DevBuf tab, tmin, slot_id, blv, scal, excl;
	DevBuf name_off, name_len, name_pos, seq_len, names;
	struct PafStream *stream = nullptr; // a streamed ingest in progress, or the report of the last one (mahip_paf_stream_*)
	size_t nbytes = 0, name_bytes = 0;
	uint32_t n_seq = 0;
	bool loaded = false;
	// what the last parse decided and counted (mahip_paf_last / mahip_paf_cols_download: host bookkeeping, read-only)
	bool parsed = false;
	mahip_paf_report_t rep = {};
	std::vector<uint8_t> odd_snap; // mahip_paf_keep_odd: per line, flags == PF_ODD between the tile parser and k_paf_parse_odd
};

struct PafCols {
	uint8_t *flags;            // bit0 valid (>= 10 columns), bit1 stored, bit2 has column 11, bit3 rev
	uint32_t *ql, *qs, *qe, *tl, *ts, *te, *ml, *bl;
	uint32_t *tnoff, *qlen, *tlen; // target-name offset inside the line, name lengths (up to the first NUL)
	uint64_t *hq, *ht;
	uint32_t *qslot, *tslot;   // hash-table slot of the two names, later their ids
};

static PafBufs *paf_of(mahip_ctx *c)
{
	if (!c->paf) c->paf = new PafBufs();
	return (PafBufs*)c->paf;
}

static void paf_stream_free(mahip_ctx *c, PafBufs *b);
void paf_free(mahip_ctx *c)
{
	PafBufs *b = (PafBufs*)c->paf;
	if (!b) return;
	paf_stream_free(c, b);
	DevBuf *all[] = { &b->text, &b->lstart, &b->tile, &b->glast, &b->gmax, &b->tfirst, &b->flags, &b->tnoff, &b->qlen, &b->tlen, &b->hq, &b->ht, &b->qslot, &b->tslot, &b->tab, &b->tmin,
		&b->slot_id, &b->blv, &b->scal, &b->excl, &b->name_off, &b->name_len, &b->name_pos, &b->seq_len, &b->names };
	for (DevBuf *d : all) dev_free(c, *d);
	for (int k = 0; k < 8; ++k) dev_free(c, b->num[k]);
	delete b;
	c->paf = nullptr;
}

// ------------------------------------------------------------------------------------------------ per-line parse

#define FNV_OFF 0xcbf29ce484222325ull
#define FNV_PRIME 0x100000001b3ull

// strtol(base 10) of the bytes [beg, end) of a column, truncated to 32 bits (paf.c:41-52 through the (uint32_t) casts)
template <typename PTR>
__device__ __forceinline__ uint32_t paf_num(PTR &p, uint32_t beg, uint32_t end)
{
	uint32_t pos = beg, nd = 0;
	unsigned ch = 0;
	for (; pos < end; ++pos) { ch = p[pos]; if (!(ch == ' ' || (ch >= 0x0bu && ch <= 0x0du))) break; } // leading blanks (TAB / LF cannot occur inside a column)
	bool neg = false, ovf = false;
	if (pos < end && (ch == '+' || ch == '-')) { neg = ch == '-'; ++pos; }
	uint64_t acc = 0;
	for (; pos < end; ++pos, ++nd) {
		const unsigned d = (unsigned)p[pos] - '0';
		if (d >= 10u) break; // junk (or a NUL) ends the number
		if (nd < 18) acc = acc * 10 + d; // 18 digits cannot overflow 63 bits
		else {
			const uint64_t lim = neg ? 0x8000000000000000ull : 0x7fffffffffffffffull;
			if (ovf || acc > (lim - d) / 10) ovf = true; else acc = acc * 10 + d;
		}
	}
	return ovf ? (neg ? 0u : 0xffffffffu) : (uint32_t)(neg ? (uint64_t)0 - acc : acc); // LONG_MIN -> 0, LONG_MAX -> 0xffffffff
}

// ---- name keys.  A name of 1..8 bytes IS its key (the bytes, zero-padded: names are C strings, so no byte of them is 0 and the padded word is unique);
// any other name (empty, or longer) gets a 64-bit hash of its length and its 8-byte words.  A file whose names are all short therefore has an EXACT
// dictionary without a single text comparison (k_dict_insert_short); as soon as one name is long the table is keyed by the mixed key and every probe
// compares the text (k_dict_insert).  key_mix spreads either kind over the table.
#define KEY_SEED 0x9e3779b97f4a7c15ull
#define KEY_LENMUL 0xff51afd7ed558ccdull
#define KEY_MUL 0xd6e8feb86659fd93ull
__host__ __device__ __forceinline__ uint64_t key_mix(uint64_t z) { z ^= z >> 33; z *= 0xff51afd7ed558ccdull; z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ull; z ^= z >> 33; return z; }
__host__ __device__ __forceinline__ uint64_t key_step(uint64_t h, uint64_t w) { h = (h ^ w) * KEY_MUL; return h ^ (h >> 29); }
__host__ __device__ __forceinline__ bool key_is_short(uint32_t len) { return len - 1u < 8u; }

// key of a name column up to its first NUL (the reference handles names as C strings); *len = its bytes.  Byte-wise form (any PTR): the slow paths
template <typename PTR>
__device__ __forceinline__ uint64_t paf_name(PTR &p, uint32_t beg, uint32_t end, uint32_t *len)
{
	uint32_t pos = beg;
	for (; pos < end; ++pos) if (p[pos] == 0) break;
	const uint32_t l = pos - beg;
	*len = l;
	uint64_t h = KEY_SEED ^ ((uint64_t)l * KEY_LENMUL), w = 0;
	for (uint32_t k = 0; k < l; ++k) {
		w |= (uint64_t)p[beg + k] << (8 * (k & 7));
		if ((k & 7) == 7 || k + 1 == l) { if (l <= 8) return w; h = key_step(h, w); w = 0; }
	}
	return h;
}

// the column starts of the block's 256 lines in LDS, column-major: lane i's k-th entry sits at [k][i], so a wave's accesses never share a bank
struct FsCols {
	uint32_t *b;
	__device__ __forceinline__ uint32_t &operator[](uint32_t k) const { return b[k * 256u]; }
};
// column starts: fs[k] = position after the k-th TAB of the line (k < 12); returns the number of TABs
template <typename PTR>
__device__ __forceinline__ uint32_t paf_tabs(PTR &p, uint32_t l, FsCols fs)
{
	uint32_t t = 0;
	fs[0] = 0;
	for (uint32_t pos = 0; pos < l; ++pos)
		if (p[pos] == '\t') { ++t; if (t < 12) fs[t] = pos + 1; }
	return t;
}

struct PafLine { uint32_t valid, hasbl, rev, ql, qs, qe, tl, ts, te, ml, bl, tnoff, qlen, tlen; uint64_t hq, ht; };

// One line: first the column starts (one pass over the bytes, starts kept in LDS), then each column with straight-line
// code -- every lane is in the same routine at the same time, only the trip counts differ.
template <typename PTR>
__device__ __forceinline__ void paf_line(PTR p, uint32_t l, FsCols fs /* LDS, 12 entries */, PafLine &o)
{
	if (l > 1 && p[l - 1] == '\r') --l;
	uint32_t t = paf_tabs(p, l, fs);
	++t; // columns
	if (t < 12) fs[t] = l + 1; // end sentinel: column k is [fs[k], fs[k+1] - 1)
	o.valid = t >= 10; o.hasbl = t >= 11;
	o.rev = 0; o.ql = o.qs = o.qe = o.tl = o.ts = o.te = o.ml = o.bl = o.tnoff = o.qlen = o.tlen = 0; o.hq = o.ht = 0;
	if (!o.valid) return; // the reference fills the columns it finds and drops the record: nothing of it is ever used
	o.hq = paf_name(p, fs[0], fs[1] - 1, &o.qlen);
	o.ql = paf_num(p, fs[1], fs[2] - 1);
	o.qs = paf_num(p, fs[2], fs[3] - 1);
	o.qe = paf_num(p, fs[3], fs[4] - 1);
	o.rev = fs[4] < fs[5] - 1 && p[fs[4]] == '-';
	o.tnoff = fs[5];
	o.ht = paf_name(p, fs[5], fs[6] - 1, &o.tlen);
	o.tl = paf_num(p, fs[6], fs[7] - 1);
	o.ts = paf_num(p, fs[7], fs[8] - 1);
	o.te = paf_num(p, fs[8], fs[9] - 1);
	o.ml = paf_num(p, fs[9], fs[10] - 1) & 0x7fffffffu;
	if (o.hasbl) o.bl = paf_num(p, fs[10], fs[11] - 1);
}

// the `bl` a 10-column line inherits: value of the nearest earlier line with an 11th column (paf.c leaves the field alone)
__global__ __launch_bounds__(256) void k_paf_bl_compact(const uint32_t *__restrict__ f_hasbl, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ bl, uint32_t L, uint32_t *__restrict__ blv)
{
	uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < L && f_hasbl[i]) blv[pos[i]] = bl[i];
}
__global__ __launch_bounds__(256) void k_bl_fill_from(const uint32_t *__restrict__ f_hasbl, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ blv, uint32_t L, uint32_t *__restrict__ bl, uint32_t before)
{ // before: what a line in front of the text's first 11-column line inherits -- 0 at the start of the file, the previous ranges' last bl in a range that does not start it
	uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < L && !f_hasbl[i]) bl[i] = pos[i] ? blv[pos[i] - 1] : before;
}

// ------------------------------------------------------------------------------------------------ tile parser (round 6)
// Round 5 parsed a line per lane with paf_line, every byte twice in divergent loops: bound by the CU's ONE scalar unit (profiles/r04_sq_counters_cfg4.txt:
// 12.6 ms per 100 M lines).  This one has no per-byte loop at all:
//   * the text is cut into tiles of K KiB (K from the mean line length: about 240 lines a tile); a tile owns the lines that END in it and keeps the up to
//     960 bytes in front of it in LDS as well, where its first line may start;
//   * while the 16-byte pieces travel from HBM to LDS their TABs and newlines are found by SWAR compares and leave as one BIT per byte (two 2-KiB arrays);
//   * newline ranks (a block scan of popcounts) give every line of the tile a lane; the lane finds its 11 column ends with count-trailing-zeros on a
//     64-bit window of the TAB bits and converts each number from the 8 bytes at its start: XOR '0', shift the digits to the top, check "all <= 9" and fold
//     them with three multiply-adds per half -- straight-line code, every lane in step;
//   * anything the straight line does not cover -- a sign, blanks, junk behind the digits, more than 8 digits, an empty column, a NUL in a name, a name of more
//     than 64 bytes, a line that starts more than 960 bytes in front of its tile -- marks the line ODD, and k_paf_parse_odd runs the byte-wise routine above
//     on exactly those lines (the reference's strtol semantics live there, and only there).
// Line i is the line that ends with the i-th newline; a text without a final newline gets a virtual one at position n.
#define PAF_GRAN 1024u        // granule of the newline census: one wave, 64 x 16 bytes
#define PAF_OVER 960u         // bytes in front of a tile that are staged with it
#define PAF_BGRP 12           // log2 of the granules per group of the "last newline" look-up
#define PF_ODD 0x80u          // flags: the line waits for k_paf_parse_odd
#define PF_QCONT 0x10u        // flags: stored line whose query name (short or long) equals that of the stored line in front of it
#define PC_LONG CT_NSHORT     // stored lines with a name that is not 1..8 bytes
#define PC_ODD CT_NASYMM

__device__ __forceinline__ uint32_t eq_mask(uint32_t v, uint32_t c4) { v ^= c4; const uint32_t t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu; return ~(t | v | 0x7F7F7F7Fu); } // 0x80 in every byte of v that equals c
// the flags of two masks as one byte: newline flags -> bits 0..3, TAB flags -> bits 4..7 (one multiply gathers both: the partial products land on 32 distinct bits)
__device__ __forceinline__ uint32_t nib8(uint32_t m_nl, uint32_t m_tab) { return (((m_nl >> 7) | (m_tab >> 3)) * 0x204081u) >> 21 & 0xFFu; }
// TAB bits (low half) and newline bits (high half) of a 16-byte piece
__device__ __forceinline__ uint32_t masks16(const uint4 v)
{
	const uint32_t a = nib8(eq_mask(v.x, 0x0A0A0A0Au), eq_mask(v.x, 0x09090909u)), b = nib8(eq_mask(v.y, 0x0A0A0A0Au), eq_mask(v.y, 0x09090909u));
	const uint32_t c = nib8(eq_mask(v.z, 0x0A0A0A0Au), eq_mask(v.z, 0x09090909u)), d = nib8(eq_mask(v.w, 0x0A0A0A0Au), eq_mask(v.w, 0x09090909u));
	const uint32_t nl = (a & 15u) | (b & 15u) << 4 | (c & 15u) << 8 | (d & 15u) << 12, tb = a >> 4 | (b >> 4) << 4 | (c >> 4) << 8 | (d >> 4) << 12;
	return tb | nl << 16;
}

// granule g = bytes [1024 g, 1024 g + 1024), one wave: cnt[g] = its newlines, last[g] = offset of the byte behind its last newline (0: it has none).
// (The text ends with a newline -- the host appends one to a text that does not -- and is followed by zeros up to the next 16 bytes.)
#define PAF_GC_PER_WAVE 8u
__global__ __launch_bounds__(256) void k_paf_gran_count(const unsigned char *__restrict__ text, size_t n, uint32_t n_gran, uint32_t *__restrict__ cnt, uint32_t *__restrict__ last)
{ // a wave takes PAF_GC_PER_WAVE consecutive granules and has all their loads in flight at once (one granule per wave: 5.9 M waves of one load each, 1.4 ms for 6 GB)
	const uint32_t g0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * PAF_GC_PER_WAVE, lane = threadIdx.x & 63;
	if (g0 >= n_gran) return; // the whole wave
	uint4 v[PAF_GC_PER_WAVE];
#pragma unroll
	for (uint32_t k = 0; k < PAF_GC_PER_WAVE; ++k) {
		const size_t off = (size_t)(g0 + k) * PAF_GRAN + lane * 16u;
		v[k] = off < n ? *(const uint4*)(text + off) : make_uint4(0, 0, 0, 0);
	}
#pragma unroll
	for (uint32_t k = 0; k < PAF_GC_PER_WAVE; ++k) {
		const uint32_t g = g0 + k;
		if (g >= n_gran) break; // the whole wave
		const uint32_t mx = eq_mask(v[k].x, 0x0A0A0A0Au), my = eq_mask(v[k].y, 0x0A0A0A0Au), mz = eq_mask(v[k].z, 0x0A0A0A0Au), mw = eq_mask(v[k].w, 0x0A0A0A0Au);
		const uint32_t c = wv_sum_u32((uint32_t)(__popc(mx) + __popc(my) + __popc(mz) + __popc(mw)));
		const unsigned long long has = __ballot((mx | my | mz | mw) != 0);
		if (lane == 0) { cnt[g] = c; if (!has) last[g] = 0; }
		if (has && (int)lane == 63 - __clzll((long long)has)) { // the lane with the granule's last newline: byte index of its highest flag + 1
			const uint32_t w = mw ? 3u : mz ? 2u : my ? 1u : 0u, m = mw ? mw : mz ? mz : my ? my : mx;
			last[g] = lane * 16u + w * 4u + ((31u - (uint32_t)__clz((int)m)) >> 3) + 1u;
		}
	}
}
// bmax[b] = byte behind the last newline of granules [4096 b, 4096 b + 4096) (0: none), one wave per group
__global__ __launch_bounds__(64) void k_paf_gran_bmax(const uint32_t *__restrict__ last, uint32_t n_gran, unsigned long long *__restrict__ bmax)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	const long g_lo = (long)b << PAF_BGRP;
	long g_hi = g_lo + (1l << PAF_BGRP); if (g_hi > (long)n_gran) g_hi = (long)n_gran;
	unsigned long long r = 0;
	for (long top = g_hi; top > g_lo && r == 0; top -= 64) { // 64 granules per step, from the back
		const long g = top - 1 - (long)lane;
		const uint32_t l = g >= g_lo ? last[g] : 0u;
		const unsigned long long has = __ballot(l != 0);
		if (has) { const int src = __ffsll((long long)has) - 1; const uint32_t lv = wv_bcast(l, src); r = (unsigned long long)(top - 1 - src) * PAF_GRAN + lv; }
	}
	if (lane == 0) bmax[b] = r;
}
// first[t] = start of the first line that ends in tile t = byte behind the last newline in front of the tile (0: the text starts it)
__global__ __launch_bounds__(256) void k_paf_tile_first(const uint32_t *__restrict__ last, const unsigned long long *__restrict__ bmax, uint32_t K, uint32_t n_tiles, unsigned long long *__restrict__ first)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= n_tiles) return;
	long g = (long)t * (long)K - 1;
	const long g_lo = g >= 0 ? (g >> PAF_BGRP) << PAF_BGRP : 0;
	unsigned long long r = 0;
	for (; g >= g_lo; --g) { const uint32_t l = last[g]; if (l) { r = (unsigned long long)g * PAF_GRAN + l; break; } }
	if (r == 0) for (long b = (g_lo >> PAF_BGRP) - 1; b >= 0; --b) if (bmax[b]) { r = bmax[b]; break; }
	first[t] = r;
}

struct TileArgs {
	const unsigned char *text; size_t n; // (ends with a newline, zeros behind it)
	uint32_t K, n_gran, n_tiles, L;
	const uint32_t *goff;            // [n_gran + 1] newlines in front of every granule
	const unsigned long long *first; // [n_tiles]
	int min_span, min_match;
};

// the 8 bytes at LDS offset pos (any alignment) as lo | hi << 32
__device__ __forceinline__ uint64_t lds_get8(const uint32_t *__restrict__ w, uint32_t pos)
{
	const uint32_t i = pos >> 2, sh = (pos & 3u) * 8u;
	const uint32_t w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
	const uint32_t lo = (uint32_t)(((uint64_t)w1 << 32 | w0) >> sh), hi = (uint32_t)(((uint64_t)w2 << 32 | w1) >> sh);
	return (uint64_t)hi << 32 | lo;
}
// distance from pos to the first TAB at or behind it: exact below 33 (two words of bits) / below 64 (three), at least that otherwise
__device__ __forceinline__ uint32_t tab_dist2(const uint32_t *__restrict__ tb, uint32_t pos)
{
	const uint32_t i = pos >> 5, sh = pos & 31u;
	const uint64_t x = ((uint64_t)tb[i + 1] << 32 | tb[i]) >> sh;
	return x ? (uint32_t)__builtin_ctzll(x) : 64u - sh; // (none among the 64 - sh >= 33 bits the two words hold)
}
__device__ __forceinline__ uint32_t tab_dist3(const uint32_t *__restrict__ tb, uint32_t pos)
{
	const uint32_t i = pos >> 5, sh = pos & 31u;
	uint64_t x = ((uint64_t)tb[i + 1] << 32 | tb[i]) >> sh;
	if (sh) x |= (uint64_t)tb[i + 2] << (64u - sh);
	return x ? (uint32_t)__builtin_ctzll(x) : 64u;
}
// a column of 1..8 digits at v (its first byte lowest) -> its value; *bad collects 0x80 flags of bytes that are not digits
__device__ __forceinline__ uint32_t num8(uint64_t v, uint32_t len, uint32_t *bad)
{
	v ^= 0x3030303030303030ull;            // '0'..'9' -> 0..9
	v <<= 8u * (8u - len);                 // the column's last digit into the top byte; what stood behind the column falls out, leading zeros come in
	uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
	*bad |= (lo + 0x76767676u) | lo | (hi + 0x76767676u) | hi; // a byte > 9 sets its top bit (a carry can only leave a byte that has set it already)
	lo = (lo & 0x00ff00ffu) * 10u + ((lo >> 8) & 0x00ff00ffu); // d0 d1 | d2 d3
	lo = (lo & 0xffffu) * 100u + (lo >> 16);
	hi = (hi & 0x00ff00ffu) * 10u + ((hi >> 8) & 0x00ff00ffu);
	hi = (hi & 0xffffu) * 100u + (hi >> 16);
	return lo * 10000u + hi;
}
// key of the name [pos, pos + len) in LDS (paf_name's function, on words); *nul: a NUL among its bytes
__device__ __forceinline__ uint64_t lds_name_key(const uint32_t *__restrict__ w, uint32_t pos, uint32_t len, uint32_t *nul)
{
	if (len <= 8) {
		const uint64_t m = len == 8 ? ~0ull : (1ull << (8u * len)) - 1ull;
		const uint64_t v = lds_get8(w, pos), f = v | ~m;
		*nul |= ((f - 0x0101010101010101ull) & ~f & 0x8080808080808080ull) != 0;
		return len ? (v & m) : KEY_SEED;
	}
	uint64_t h = KEY_SEED ^ ((uint64_t)len * KEY_LENMUL);
	for (uint32_t k = 0; k < len; k += 8) {
		const uint32_t rem = len - k;
		const uint64_t m = rem >= 8 ? ~0ull : (1ull << (8u * rem)) - 1ull;
		const uint64_t v = lds_get8(w, pos + k), f = v | ~m;
		*nul |= ((f - 0x0101010101010101ull) & ~f & 0x8080808080808080ull) != 0;
		h = key_step(h, v & m);
	}
	return h;
}

#define PAF_TILE_WAVES 1 // __launch_bounds__' second argument (waves per SIMD the register allocation has to leave room for)
// the block's dynamic LDS (declared outside the template: the CPU test build's g++ gets an extern thread_local declared inside a template wrong)
extern __shared__ __attribute__((aligned(16))) unsigned char s_text[];
template <int CH> // a block stages up to CH * 16 KiB of text: CH * 64 bytes per thread in the newline ranking
__global__ __launch_bounds__(256, PAF_TILE_WAVES) void k_paf_parse_tile(const TileArgs a, PafCols o, uint64_t *__restrict__ lstart, unsigned long long *__restrict__ ctr)
{
	constexpr uint32_t REG = (uint32_t)CH * 16384u;
	// s_text: the text, REG + 32; behind it:
	uint16_t *s_tb = (uint16_t*)(s_text + REG + 32);        // REG / 16 + 8: TAB bits, one u16 per 16-byte piece
	uint16_t *s_nb = s_tb + REG / 16 + 8;                   // the same for newlines
	uint32_t *s_lend = (uint32_t*)(s_nb + REG / 16 + 8);    // [0] end of the line in front of the batch, [1 + j] newline of the batch's j-th line
	__shared__ uint32_t s_w[4];
	const uint32_t *tw = (const uint32_t*)s_text, *tb = (const uint32_t*)s_tb;
	const unsigned lane = threadIdx.x & 63;
	uint32_t c_valid = 0, c_pass = 0, c_nobl = 0, c_long = 0, c_odd = 0;
	uint64_t c_mq = 0;
	// A block works through tiles blockIdx.x, + gridDim.x, ...; the pieces of the NEXT tile are on their way from HBM (in registers) while the lines of this one are
	// parsed: the trip to memory is paid once per block, not once per tile.
	constexpr int NP = 4 * CH; // 16-byte pieces per thread
	struct Geom { uint32_t line0, tot, len; uint64_t first, lo; bool long_first; };
	auto geom = [&](uint32_t t) {
		Geom g;
		const uint32_t g0 = t * a.K, g1 = g0 + a.K < a.n_gran ? g0 + a.K : a.n_gran;
		g.line0 = a.goff[g0]; g.tot = a.goff[g1] - g.line0; // the lines that end in this tile
		const uint64_t tb0 = (uint64_t)g0 * PAF_GRAN, te0 = (uint64_t)g1 * PAF_GRAN;
		g.first = a.first[t];
		uint64_t lo = tb0 > PAF_OVER ? tb0 - PAF_OVER : 0;
		g.long_first = g.first < lo; // the first line starts further in front than the block keeps: its bytes are not all here
		if (!g.long_first) lo = g.first;
		g.lo = lo & ~(uint64_t)63;
		g.len = g.tot ? (uint32_t)(te0 - g.lo) : 0u; // <= REG, a multiple of 64; a tile in which no line ends is not loaded at all
		return g;
	};
	uint4 pv[NP];
	auto fetch = [&](const Geom &g) {
#pragma unroll
		for (int q = 0; q < NP; ++q) {
			const uint32_t p = threadIdx.x + 256u * (uint32_t)q;
			const uint64_t off = g.lo + (uint64_t)p * 16u;
			pv[q] = p * 16u < g.len && off < a.n ? *(const uint4*)(a.text + off) : make_uint4(0, 0, 0, 0);
		}
	};
	uint32_t t = blockIdx.x;
	Geom cur = {};
	if (t < a.n_tiles) { cur = geom(t); fetch(cur); }
	for (; t < a.n_tiles; t += gridDim.x) {
		const uint32_t line0 = cur.line0, tot = cur.tot, len = cur.len;
		const uint64_t first = cur.first, lo = cur.lo;
		const bool long_first = cur.long_first;
#pragma unroll
		for (int q = 0; q < NP; ++q) {
			const uint32_t p = threadIdx.x + 256u * (uint32_t)q;
			if (p * 16u >= len) break;
			const uint64_t off = lo + (uint64_t)p * 16u;
			uint32_t m = masks16(pv[q]);
			if (off < first) m &= off + 16 <= first ? 0u : (0xffffu << (uint32_t)(first - off) & 0xffffu) * 0x10001u; // bytes of lines that ended in front of this tile
			*(uint4*)(s_text + p * 16u) = pv[q];
			s_tb[p] = (uint16_t)m; s_nb[p] = (uint16_t)(m >> 16);
		}
		if (t + gridDim.x < a.n_tiles) { cur = geom(t + gridDim.x); fetch(cur); } // in flight until the next turn of the loop
		if (tot == 0) continue; // the whole block (nothing was written, nothing is read)
		for (uint32_t p = len / 16u + threadIdx.x; p < REG / 16u; p += 256u) s_nb[p] = 0; // (the ranking below reads the whole array)
		__syncthreads();
		// ---- ranks of the newlines: thread x looks after bytes [64 CH x, 64 CH (x + 1))
		unsigned long long nlm[CH];
		uint32_t cnt = 0;
#pragma unroll
		for (int r = 0; r < CH; ++r) { nlm[r] = *(const unsigned long long*)(s_nb + 4u * (threadIdx.x * CH + r)); cnt += (uint32_t)__popcll(nlm[r]); }
		uint32_t tot_here;
		const uint32_t rank0 = block_excl_scan_256(cnt, s_w, &tot_here);
		if (threadIdx.x == 0) s_lend[0] = long_first ? 0u : (uint32_t)(first - lo) - 1u; // (a long first line never uses it)
		for (uint32_t base = 0; base < tot; base += 256u) {
			{
				uint32_t r = rank0;
#pragma unroll
				for (int q = 0; q < CH; ++q)
					for (unsigned long long m = nlm[q]; m; m &= m - 1, ++r)
						if (r - base < 256u) s_lend[1u + r - base] = (threadIdx.x * CH + q) * 64u + (uint32_t)__builtin_ctzll(m);
			}
			__syncthreads();
			const uint32_t r = base + threadIdx.x;
			const bool act = r < tot;
			const uint32_t i = line0 + r;
			uint32_t fl = 0, mine = 0, x_ps = 0, x_qlen = 0; // (x_*: where this lane's query name stands in LDS and how long it is, for the lane above)
			uint64_t hq = 0, ht = 0;
			if (act) {
				const uint32_t pe = s_lend[1u + threadIdx.x], ps = s_lend[threadIdx.x] + 1u;
				const bool lf = long_first && r == 0;
				lstart[i] = lf ? first : lo + ps;
				if (i + 1 == a.L) lstart[i + 1] = lo + pe + 1;
				bool odd = lf;
				if (!lf) {
					uint32_t e1 = pe;
					if (e1 - ps > 1 && s_text[e1 - 1] == '\r') --e1;
					// ---- column ends (all eleven first, then what they hold: converting each column as soon as its end is known -- 22 registers fewer on paper -- made hipcc
					// interleave less: 99 registers and 4.12 ms instead of 96 and 3.85; capping the registers for six waves a SIMD spills: 5.9 ms)
					uint32_t fb[11], fe[11], ncol = 0, pos = ps;
					bool more = true, amb = false;
#pragma unroll
					for (int k = 0; k < 11; ++k) {
						const bool name = k == 0 || k == 5;
						const uint32_t d = name ? tab_dist3(tb, pos) : tab_dist2(tb, pos);
						uint32_t end = pos + d;
						const bool lastc = end >= e1; // no TAB before the line ends: the last column
						amb |= more && !lastc && d >= (name ? 64u : 33u); // the window ended before the column did
						end = lastc ? e1 : end;
						fb[k] = pos; fe[k] = end;
						ncol += more;
						more = more && !lastc;
						pos = more ? end + 1u : e1;
					}
					const uint32_t valid = ncol >= 10, hasbl = ncol >= 11;
					odd = amb;
					uint32_t ql = 0, qs = 0, qe = 0, tl = 0, ts = 0, te = 0, ml = 0, bl = 0, rev = 0, tnoff = 0, qlen = 0, tlen = 0, pass = 0;
					if (valid && !amb) {
						uint32_t bad = 0, lbad = 0, nul = 0;
#define PAF_NUM(k) ({ const uint32_t l_ = fe[k] - fb[k]; lbad |= (l_ - 1u) > 7u; num8(lds_get8(tw, fb[k]), (l_ - 1u) > 7u ? 8u : l_, &bad); })
						ql = PAF_NUM(1); qs = PAF_NUM(2); qe = PAF_NUM(3);
						tl = PAF_NUM(6); ts = PAF_NUM(7); te = PAF_NUM(8);
						ml = PAF_NUM(9) & 0x7fffffffu;
						if (hasbl) bl = PAF_NUM(10);
#undef PAF_NUM
						rev = fe[4] > fb[4] && s_text[fb[4]] == '-';
						tnoff = fb[5] - ps;
						qlen = fe[0] - fb[0]; tlen = fe[5] - fb[5];
						if (qlen > 64 || tlen > 64) lbad = 1;
						else { hq = lds_name_key(tw, fb[0], qlen, &nul); ht = lds_name_key(tw, fb[5], tlen, &nul); }
						odd = (bad & 0x80808080u) != 0 || lbad || nul;
						pass = !(qe - qs < (uint32_t)a.min_span || te - ts < (uint32_t)a.min_span || (int)ml < a.min_match); // hit.c:85
					}
					if (!odd) {
						fl = valid | pass << 1 | hasbl << 2 | rev << 3;
						c_valid += valid; c_pass += pass; c_nobl += valid && !hasbl;
						if (pass) {
							const uint32_t lng = !key_is_short(qlen) || !key_is_short(tlen);
							c_long += lng;
							mine = 1; x_ps = ps; x_qlen = qlen;
							const uint64_t mq = qs > ts ? qs : ts;
							c_mq = mq > c_mq ? mq : c_mq;
						}
						o.ql[i] = ql; o.qs[i] = qs; o.qe[i] = qe; o.tl[i] = tl; o.ts[i] = ts; o.te[i] = te; o.ml[i] = ml; o.bl[i] = bl;
						o.tnoff[i] = tnoff; o.qlen[i] = qlen; o.tlen[i] = tlen; o.hq[i] = hq; o.ht[i] = ht;
					}
				}
				if (odd) { fl = PF_ODD; ++c_odd; }
			}
			// does the line continue the run of one query name?  (the lane below holds the line in front; lane 0 of a wave starts a run)
			const uint32_t p_mine = wv_prev_lane_u32(mine, 0u, lane), p_lo = wv_prev_lane_u32((uint32_t)hq, 0u, lane), p_hi = wv_prev_lane_u32((uint32_t)(hq >> 32), 0u, lane);
			const uint32_t p_len = wv_prev_lane_u32(x_qlen, 0u, lane), p_ps = wv_prev_lane_u32(x_ps, 0u, lane);
			bool cont = mine && p_mine && p_len == x_qlen && p_lo == (uint32_t)hq && p_hi == (uint32_t)(hq >> 32);
			if (cont && !key_is_short(x_qlen)) // a hashed key: the bytes decide (both names are in LDS: the one place where comparing them costs nothing)
				for (uint32_t k = 0; k < x_qlen && cont; k += 8) {
					const uint32_t rem = x_qlen - k;
					const uint64_t m = rem >= 8 ? ~0ull : (1ull << (8u * rem)) - 1ull;
					cont = ((lds_get8(tw, x_ps + k) ^ lds_get8(tw, p_ps + k)) & m) == 0;
				}
			if (cont) fl |= PF_QCONT;
			if (act) o.flags[i] = (uint8_t)fl;
			__syncthreads();
			if (base + 256u < tot) { if (threadIdx.x == 0) s_lend[0] = s_lend[256]; __syncthreads(); }
		}
	}
	blk_add_u64(&ctr[PC_VALID], c_valid);
	blk_add_u64(&ctr[PC_PASS], c_pass);
	blk_add_u64(&ctr[PC_NOBL], c_nobl);
	blk_add_u64(&ctr[PC_LONG], c_long);
	blk_add_u64(&ctr[PC_ODD], c_odd);
	blk_max_u64(&ctr[PC_MAXQS], c_mq);
}

// the lines the tile parser left (flags == PF_ODD): the byte-wise routine, straight from global memory
__global__ __launch_bounds__(256) void k_paf_parse_odd(const unsigned char *__restrict__ text, const uint64_t *__restrict__ lstart, uint32_t L, int min_span, int min_match, PafCols o,
                                                        unsigned long long *__restrict__ ctr)
{
	__shared__ uint32_t s_fs[256 * 12];
	uint32_t c_valid = 0, c_pass = 0, c_nobl = 0, c_long = 0;
	uint64_t c_mq = 0;
	for (uint32_t base = blockIdx.x * 256u; base < L; base += gridDim.x * 256u) {
		const uint32_t i = base + threadIdx.x;
		if (i >= L || o.flags[i] != PF_ODD) continue;
		const uint64_t ls = lstart[i];
		const uint32_t l = (uint32_t)(lstart[i + 1] - 1 - ls);
		PafLine r;
		const FsCols fs = { s_fs + threadIdx.x };
		paf_line(text + ls, l, fs, r);
		const uint32_t pass = r.valid && !(r.qe - r.qs < (uint32_t)min_span || r.te - r.ts < (uint32_t)min_span || (int)r.ml < min_match); // hit.c:85
		c_valid += r.valid; c_pass += pass; c_nobl += r.valid && !r.hasbl;
		o.flags[i] = (uint8_t)(r.valid | pass << 1 | r.hasbl << 2 | r.rev << 3);
		o.ql[i] = r.ql; o.qs[i] = r.qs; o.qe[i] = r.qe; o.tl[i] = r.tl; o.ts[i] = r.ts; o.te[i] = r.te; o.ml[i] = r.ml; o.bl[i] = r.bl;
		o.tnoff[i] = r.tnoff; o.qlen[i] = r.qlen; o.tlen[i] = r.tlen; o.hq[i] = r.hq; o.ht[i] = r.ht;
		if (pass) {
			c_long += !key_is_short(r.qlen) || !key_is_short(r.tlen);
			const uint64_t mq = r.qs > r.ts ? r.qs : r.ts;
			c_mq = mq > c_mq ? mq : c_mq;
		}
	}
	blk_add_u64(&ctr[PC_VALID], c_valid);
	blk_add_u64(&ctr[PC_PASS], c_pass);
	blk_add_u64(&ctr[PC_NOBL], c_nobl);
	blk_add_u64(&ctr[PC_LONG], c_long);
	blk_max_u64(&ctr[PC_MAXQS], c_mq);
}
__global__ __launch_bounds__(256) void k_paf_hasbl(const uint8_t *__restrict__ flags, uint32_t L, uint32_t *__restrict__ f_hasbl)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < L) f_hasbl[i] = flags[i] >> 2 & 1u;
}

// ------------------------------------------------------------------------------------------------ name dictionary

__device__ __forceinline__ bool name_eq(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b, uint32_t len)
{ // 8 bytes at a time (global loads need no alignment), the tail byte by byte
	uint32_t k = 0;
	for (; k + 8 <= len; k += 8) {
		unsigned long long x, y;
		__builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8);
		if (x != y) return false;
	}
	for (; k < len; ++k) if (a[k] != b[k]) return false;
	return true;
}

// (Round 3 tried 32-byte slots that carry the first 16 bytes of the name, so that the sector that answers a probe also settles the comparison: with
// agent-scope accesses to keep the eight L2s honest and a table four times the bytes it was SLOWER -- 17.0 against 11.5 ms per 100 M lines
// (profiles/r03_experiments.txt) -- and was taken out again.)
// One thread per stored line: query name, then target name.  A slot is two words: w0 = tag(32) | an occurrence (2*line + column) of the slot's name -- the
// claimant's at first, the SMALLEST seen so far in the end = the name's first appearance in the file --, info = text offset << 24 | length of the slot's name,
// written by the claimant right after its CAS: a prober that finds it compares the bytes after ONE dependent fetch; one that does not see it yet (the store is
// not ordered with the CAS, a stale line) goes the long way through the occurrence (line start, column offset, length: three more random fetches) -- both ways
// read the same bytes.
#define PAF_INFO_LEN_BITS 24
// the slot of one name occurrence (probe, insert if new); 0xffffffff: the probe sequence ran out
// (Round 6: the slot's two words sit side by side -- one 16-byte fetch answers "whose slot" and "where is its text" --, and the low half of the first word is the SMALLEST
// occurrence seen so far, kept by a 64-bit atomicMin (every writer of a slot carries the slot's tag in the high half): the separate info and tmin arrays, two of a
// probe's five random fetches, are gone.  tmin[] is written once, behind the pass (k_dict_exact_tmin), for the code that ranks the names.)
struct __attribute__((aligned(16))) XSlot { unsigned long long w0, info; };
__device__ __forceinline__ uint32_t dict_probe(const unsigned char *__restrict__ text, const uint64_t *__restrict__ lstart, const PafCols &o,
                                               XSlot *__restrict__ tab, uint32_t mask,
                                               uint64_t h, uint32_t len, uint32_t occ, uint64_t noff, uint32_t *fresh)
{
	const unsigned char *nm = text + noff;
	const uint64_t hm = key_mix(h); // (a short name's key is its bytes: mixed before it picks a slot)
	const uint32_t tag = (uint32_t)(hm >> 32);
	uint32_t s = (uint32_t)hm & mask;
	for (uint32_t probe = 0; probe < PAF_PROBE_LIMIT; ++probe, s = (s + 1) & mask) {
		// (two 64-bit words, not four 32-bit ones: a word another thread is claiming must be seen whole -- as the halves of a uint4 the CPU test build read it in two pieces, and a
		// torn tag sent the probe on to a second slot for the same name: one run of the command line in a thousand)
		const ulonglong2 raw = *(const ulonglong2*)&tab[s];
		unsigned long long e = raw.x, inf = raw.y;
		if (e == PAF_EMPTY) {
			e = atomicCAS(&tab[s].w0, PAF_EMPTY, (unsigned long long)tag << 32 | occ);
			if (e == PAF_EMPTY) {
				if (len < (1u << PAF_INFO_LEN_BITS) && noff < (1ull << (64 - PAF_INFO_LEN_BITS))) tab[s].info = noff << PAF_INFO_LEN_BITS | len;
				++*fresh;
				return s;
			}
			inf = PAF_EMPTY; // (somebody else's slot by now: its second word was not in the fetch)
		}
		if ((uint32_t)(e >> 32) == tag) {
			bool same;
			if (inf != PAF_EMPTY) same = (uint32_t)(inf & ((1u << PAF_INFO_LEN_BITS) - 1)) == len && name_eq(nm, text + (inf >> PAF_INFO_LEN_BITS), len);
			else { // the long way, through an occurrence of the slot's name (any will do: the low half only ever moves to another occurrence of the same name)
				const uint32_t r = (uint32_t)e, rl = r >> 1;
				const uint32_t rlen = (r & 1) ? o.tlen[rl] : o.qlen[rl];
				same = rlen == len && name_eq(nm, text + lstart[rl] + ((r & 1) ? o.tnoff[rl] : 0u), len);
			}
			if (same) {
				if ((uint32_t)e > occ) atomicMin(&tab[s].w0, (unsigned long long)tag << 32 | occ);
				return s;
			}
		}
	}
	return 0xffffffffu;
}
// what the rest of the dictionary code reads: tmin[slot] = first appearance of the slot's name (~0: free slot)
__global__ __launch_bounds__(256) void k_dict_exact_tmin(const XSlot *__restrict__ tab, uint32_t cap, uint32_t *__restrict__ tmin)
{
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap) { const unsigned long long e = tab[s].w0; tmin[s] = e == PAF_EMPTY ? 0xffffffffu : (uint32_t)e; }
}

// A PAF file lists a query's overlaps together (the reference's own all-vs-all pipeline writes them so; so does every overlapper that works query by
// query): the QUERY name of a line is, 49 times in 50 at BASELINE coverage, the previous line's.  A wave holds 64 consecutive lines; a lane whose query
// name equals its left neighbour's (PF_QCONT: the tile parser compared the bytes in LDS) does not probe but takes the slot of the nearest lane to its left that did (the
// head of its run: its occurrence number is the run's smallest, so tmin is right as well).  Round 2 probed once per name occurrence: 200 M probes and
// 68 GB of fetches for 100 M lines; the query column now costs one probe per run and wave.  Target names change from line to line and probe as before.
__global__ __launch_bounds__(256) void k_dict_insert(const unsigned char *__restrict__ text, const uint64_t *__restrict__ lstart, uint32_t L, PafCols o,
                                                      XSlot *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ ctr)
{
	uint32_t fail = 0, fresh = 0;
	const unsigned lane = threadIdx.x & 63;
	for (uint32_t base = blockIdx.x * 256u; base < L; base += gridDim.x * 256u) { // wave-uniform: the lanes talk to each other below
		const uint32_t i = base + threadIdx.x;
		const uint32_t fl = i < L ? o.flags[i] : 0u;
		const bool stored = (fl & 2u) != 0;
		const uint64_t ls = stored ? lstart[i] : 0;
		const uint64_t hq = stored ? o.hq[i] : 0;
		const uint32_t qlen = stored ? o.qlen[i] : 0;
		// does this line continue its left neighbour's run of one query name?
		const int stored_l = __shfl_up((int)stored, 1, 64);
		const bool cont = stored && lane > 0 && stored_l && (fl & PF_QCONT) != 0;
		uint32_t qslot = 0xffffffffu;
		if (stored && !cont) qslot = dict_probe(text, lstart, o, tab, mask, hq, qlen, i * 2u, ls, &fresh);
		const unsigned long long heads = __ballot(stored && !cont);
		{ // a continuing lane: the slot of the nearest head to its left (there is one: lane 0 never continues)
			const unsigned long long left = heads & ((1ull << lane) - 1ull);
			const int src = left ? 63 - __builtin_clzll(left) : (int)lane;
			const uint32_t got = __shfl(qslot, src, 64);
			if (cont) qslot = got;
		}
		if (stored) {
			const uint32_t tslot = dict_probe(text, lstart, o, tab, mask, o.ht[i], o.tlen[i], i * 2u + 1u, ls + o.tnoff[i], &fresh);
			if (qslot == 0xffffffffu || tslot == 0xffffffffu) fail = 1;
			o.qslot[i] = qslot; o.tslot[i] = tslot;
		}
	}
	blk_add_u64(&ctr[PC_OVERFLOW], fail);
	blk_add_u64(&ctr[PC_DISTINCT], fresh);
}

// ---- the dictionary of a file whose names are all 1..8 bytes (PC_LONG == 0): the key IS the name, so a slot that holds the key holds the name -- no text is
// compared and none is fetched.  Slot = 16 bytes { key, ~(smallest occurrence), - }: all zero = free, claimed by a 64-bit CAS on the key; the occurrence word is
// kept by atomicMax of the complement (so that zeroed memory is "none yet") and a probe touches it only when its own occurrence is smaller than what the same
// 16-byte fetch showed.  One random fetch per name occurrence (round 5's probe: five -- slot word, info word, the first inserter's text, tmin, own text).
// Run heads come from the parser (PF_QCONT), which compared the keys while it had them.
struct __attribute__((aligned(16))) DSlot { unsigned long long key; uint32_t inv_occ, pad; };
__device__ __forceinline__ uint32_t dict_probe_short(DSlot *__restrict__ tab, uint32_t mask, uint64_t key, uint32_t occ, uint32_t *fresh)
{
	uint32_t s = (uint32_t)key_mix(key) & mask;
	for (uint32_t probe = 0; probe < PAF_PROBE_LIMIT; ++probe, s = (s + 1) & mask) {
		const ulonglong2 e = *(const ulonglong2*)&tab[s]; // (64-bit words: a key being claimed is seen whole or not at all, see dict_probe)
		unsigned long long k = e.x;
		uint32_t seen = (uint32_t)e.y;
		if (k == 0) {
			k = atomicCAS(&tab[s].key, 0ull, (unsigned long long)key);
			if (k == 0) { ++*fresh; k = key; }
			seen = 0;
		}
		if (k == key) {
			if (seen < ~occ) atomicMax(&tab[s].inv_occ, ~occ);
			return s;
		}
	}
	return 0xffffffffu;
}
__global__ __launch_bounds__(256) void k_dict_insert_short(PafCols o, uint32_t L, DSlot *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ ctr)
{
	uint32_t fail = 0, fresh = 0;
	const unsigned lane = threadIdx.x & 63;
	for (uint32_t base = blockIdx.x * 256u; base < L; base += gridDim.x * 256u) { // wave-uniform
		const uint32_t i = base + threadIdx.x;
		const uint32_t fl = i < L ? o.flags[i] : 0u;
		const bool stored = (fl & 2u) != 0;
		const bool head = stored && (!(fl & PF_QCONT) || lane == 0);
		uint32_t qslot = 0xffffffffu;
		if (head) qslot = dict_probe_short(tab, mask, o.hq[i], i * 2u, &fresh);
		const unsigned long long heads = __ballot(head);
		{ // a continuing lane: the slot of the nearest head to its left (lane 0 is one whenever it is stored)
			const unsigned long long left = heads & ((1ull << lane) - 1ull);
			const int src = left ? 63 - __builtin_clzll(left) : (int)lane;
			const uint32_t got = __shfl(qslot, src, 64);
			if (stored && !head) qslot = got;
		}
		if (stored) {
			const uint32_t tslot = dict_probe_short(tab, mask, o.ht[i], i * 2u + 1u, &fresh);
			if (qslot == 0xffffffffu || tslot == 0xffffffffu) fail = 1;
			o.qslot[i] = qslot; o.tslot[i] = tslot;
		}
	}
	blk_add_u64(&ctr[PC_OVERFLOW], fail);
	blk_add_u64(&ctr[PC_DISTINCT], fresh);
}
// what the rest of the dictionary code reads: tmin[slot] = first appearance of the slot's name (~0: free slot)
__global__ __launch_bounds__(256) void k_dict_short_tmin(const DSlot *__restrict__ tab, uint32_t cap, uint32_t *__restrict__ tmin)
{
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap) tmin[s] = tab[s].key ? ~tab[s].inv_occ : 0xffffffffu;
}

// ---- -R (ma_hit_no_cont, hit.c:38-68) on the parsed columns: reads that are clearly contained are excluded BEFORE ids are given out
// (hit.c:86), so the exclusion is a property of NAMES: a line's verdict flags the name's table slot, lines that touch a flagged name are
// dropped, and first appearances are taken over the lines that are left.
__global__ __launch_bounds__(256) void k_paf_nocont(PafCols o, uint32_t L, int max_hang, float int_frac, uint8_t *__restrict__ excl)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < L; i += gridDim.x * 256u) {
		if (!(o.flags[i] & 2)) continue;
		const int v = mc_no_cont(o.ql[i], o.qs[i], o.qe[i], o.tl[i], o.ts[i], o.te[i], o.flags[i] >> 3 & 1, max_hang, int_frac);
		if (v == 1) excl[o.tslot[i]] = 1;
		else if (v == 2) excl[o.qslot[i]] = 1;
	}
}
__global__ __launch_bounds__(256) void k_paf_refilter(PafCols o, uint32_t L, const uint8_t *__restrict__ excl, uint32_t *__restrict__ tmin, unsigned long long *__restrict__ ctr)
{
	uint32_t pass = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < L; i += gridDim.x * 256u) {
		if (!(o.flags[i] & 2)) continue;
		const uint32_t qs = o.qslot[i], ts = o.tslot[i];
		if (excl[qs] || excl[ts]) { o.flags[i] &= (uint8_t)~2u; continue; }
		atomicMin(&tmin[qs], i * 2u); atomicMin(&tmin[ts], i * 2u + 1u);
		++pass;
	}
	blk_add_u64(&ctr[PC_PASS], pass);
}
__global__ __launch_bounds__(256) void k_excl_count(const uint8_t *__restrict__ excl, uint32_t cap, unsigned long long *__restrict__ ctr)
{
	uint32_t n = 0;
	for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < cap; s += gridDim.x * 256u) n += excl[s];
	blk_add_u64(&ctr[PC_VALID], n);
}

// a name gets an id if some STORED line carries it (with -R a name may sit in the table without such a line); tmin is ~0 in free slots as well
__global__ __launch_bounds__(256) void k_dict_flag(const uint32_t *__restrict__ tmin, uint32_t cap, uint32_t *__restrict__ keep)
{
	uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap) keep[s] = tmin[s] != 0xffffffffu;
}
__global__ __launch_bounds__(256) void k_dict_collect(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ tmin, uint32_t cap,
                                                       uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap && keep[s]) { key[pos[s]] = tmin[s]; val[pos[s]] = s; }
}
// names sorted by first appearance: rank = id (sdict.c:27-45); first-seen length, where the name's bytes are
__global__ __launch_bounds__(256) void k_dict_assign(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t R, const uint64_t *__restrict__ lstart, PafCols o,
                                                      uint32_t *__restrict__ slot_id, uint32_t *__restrict__ seq_len, uint64_t *__restrict__ name_off, uint32_t *__restrict__ name_len,
                                                      uint32_t *__restrict__ keep)
{
	uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= R) return;
	const uint32_t occ = (uint32_t)key[j], line = occ >> 1, col = occ & 1;
	slot_id[val[j]] = j;
	seq_len[j] = col ? o.tl[line] : o.ql[line];
	name_off[j] = lstart[line] + (col ? o.tnoff[line] : 0u);
	const uint32_t len = col ? o.tlen[line] : o.qlen[line];
	name_len[j] = len;
	keep[j] = len + 1;
}
__global__ __launch_bounds__(256) void k_dict_names(const unsigned char *__restrict__ text, const uint64_t *__restrict__ name_off, const uint32_t *__restrict__ name_len,
                                                     const uint32_t *__restrict__ name_pos, uint32_t R, char *__restrict__ out)
{
	uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= R) return;
	const unsigned char *s = text + name_off[j];
	char *d = out + name_pos[j];
	const uint32_t len = name_len[j];
	for (uint32_t k = 0; k < len; ++k) d[k] = (char)s[k];
	d[len] = 0;
}

// ------------------------------------------------------------------------------------------------ the ranks' name tables -> one dictionary
// Sharded ingest (host/ingest_sharded.c, SURVEY 8e "ingest routing, option B"): every rank parses its own byte range of the text and holds the distinct names
// of that range with the GLOBAL occurrence number (2 x line in the whole file + column) of their first appearance there.  The tables of all ranks are gathered
// (rows + name bytes), every rank inserts all of them into one table -- minimum occurrence per name, first-seen length riding in the low word -- and sorts the
// distinct names by that minimum: the same ids on every rank, the ids the reference's sequential reader hands out (sdict.c:27-45).
struct NameRow { uint32_t occ, seq_len, name_len, name_pos; }; // one distinct name of one rank's range; name_pos: offset in that rank's block of name bytes

__device__ __forceinline__ uint64_t fnv_bytes(const unsigned char *__restrict__ p, uint32_t len)
{
	uint64_t h = FNV_OFF;
	for (uint32_t k = 0; k < len; ++k) h = (h ^ p[k]) * FNV_PRIME;
	return h;
}
// row t = rank (t / stride_rows), index (t % stride_rows); its bytes: blobs + rank * stride_bytes + name_pos
__global__ __launch_bounds__(256) void k_dict_merge(const NameRow *__restrict__ rows, const unsigned char *__restrict__ blobs, const uint32_t *__restrict__ n_rows /* per rank */, int world,
                                                     uint32_t stride_rows, size_t stride_bytes, unsigned long long *__restrict__ tab, unsigned long long *__restrict__ gkey, uint32_t mask,
                                                     uint32_t *__restrict__ slot_of, unsigned long long *__restrict__ ctr)
{
	uint32_t fail = 0;
	for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)world * stride_rows; t += (size_t)gridDim.x * 256) {
		const uint32_t rk = (uint32_t)(t / stride_rows), j = (uint32_t)(t % stride_rows);
		if (j >= n_rows[rk]) continue;
		const NameRow r = rows[t];
		const unsigned char *nm = blobs + (size_t)rk * stride_bytes + r.name_pos;
		const uint64_t h = fnv_bytes(nm, r.name_len);
		const uint32_t tag = (uint32_t)(h >> 32);
		uint32_t s = (uint32_t)h & mask, got = 0xffffffffu;
		for (uint32_t probe = 0; probe < PAF_PROBE_LIMIT; ++probe, s = (s + 1) & mask) {
			unsigned long long e = tab[s];
			if (e == PAF_EMPTY) {
				e = atomicCAS(&tab[s], PAF_EMPTY, (unsigned long long)tag << 32 | (uint32_t)t);
				if (e == PAF_EMPTY) { got = s; break; }
			}
			if ((uint32_t)(e >> 32) == tag) { // the claimant's row is part of the gathered (read-only) input: comparable at once
				const uint32_t t2 = (uint32_t)e, rk2 = t2 / stride_rows;
				const NameRow r2 = rows[t2];
				if (r2.name_len == r.name_len && name_eq(nm, blobs + (size_t)rk2 * stride_bytes + r2.name_pos, r.name_len)) { got = s; break; }
			}
		}
		if (got == 0xffffffffu) { fail = 1; continue; }
		atomicMin(&gkey[got], (unsigned long long)r.occ << 32 | r.seq_len); // first appearance in the whole file, and the length seen there
		slot_of[t] = got;
	}
	blk_add_u64(&ctr[PC_OVERFLOW], fail);
}
__global__ __launch_bounds__(256) void k_merge_flag(const unsigned long long *__restrict__ tab, uint32_t cap, uint32_t *__restrict__ keep)
{
	uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap) keep[s] = tab[s] != PAF_EMPTY;
}
__global__ __launch_bounds__(256) void k_merge_collect(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, const unsigned long long *__restrict__ gkey, uint32_t cap,
                                                        uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap && keep[s]) { key[pos[s]] = gkey[s] >> 32; val[pos[s]] = s; }
}
// id i = the i-th name by first appearance: its table slot, length, where its bytes are, how long they are
__global__ __launch_bounds__(256) void k_merge_assign(const uint32_t *__restrict__ val, uint32_t R, const unsigned long long *__restrict__ tab, const unsigned long long *__restrict__ gkey,
                                                       const NameRow *__restrict__ rows, uint32_t stride_rows, size_t stride_bytes, uint32_t *__restrict__ gid_of_slot,
                                                       uint32_t *__restrict__ seq_len, uint64_t *__restrict__ name_off, uint32_t *__restrict__ name_len, uint32_t *__restrict__ keep)
{
	uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= R) return;
	const uint32_t s = val[i], t = (uint32_t)tab[s];
	const NameRow r = rows[t];
	gid_of_slot[s] = i;
	seq_len[i] = (uint32_t)gkey[s];
	name_off[i] = (uint64_t)(t / stride_rows) * stride_bytes + r.name_pos;
	name_len[i] = r.name_len;
	keep[i] = r.name_len + 1;
}
// this rank's table slot -> global id, through the slot's local id and the row it became
__global__ __launch_bounds__(256) void k_merge_map(const uint32_t *__restrict__ keep_local /* slot in use */, const uint32_t *__restrict__ slot_id /* slot -> local id */, uint32_t cap,
                                                    const uint32_t *__restrict__ slot_of, uint32_t row0, const uint32_t *__restrict__ gid_of_slot, uint32_t *__restrict__ out)
{
	uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap && keep_local[s]) out[s] = gid_of_slot[slot_of[row0 + slot_id[s]]];
}
__global__ __launch_bounds__(256) void k_name_rows(const uint64_t *__restrict__ key /* sorted local first appearances */, uint32_t R, uint32_t occ_base, const uint32_t *__restrict__ seq_len,
                                                    const uint32_t *__restrict__ name_len, const uint32_t *__restrict__ name_pos, NameRow *__restrict__ out)
{
	uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j < R) { NameRow r; r.occ = (uint32_t)key[j] + occ_base; r.seq_len = seq_len[j]; r.name_len = name_len[j]; r.name_pos = name_pos[j]; out[j] = r; }
}

// ------------------------------------------------------------------------------------------------ records

// ids + record slots + records in ONE pass (round 5 took three launches -- ids, a scan, records -- and read the columns twice):
// a tile of 1 024 lines looks up its ids, counts its records, learns where they go from the tiles in front of it (chained look-back, scan.hip) and writes them.
// A lane has a LINE (row r of the tile = lines 64 r .. 64 r + 63, wave w takes rows w, w + 4, ...): a line's 32 or 64 bytes of records leave from one lane, so the
// lanes of a store instruction fill neighbouring 64-byte stretches (four lines per lane, as the first version had it, put them 256 bytes apart: 4.7 ms against
// the 4.1 of the three launches it replaced).
#define EM_ROWS 16u // rows per tile: a tile draws ONE ticket from one word (12 - 17 ns each, serial): 1 row 5.57 ms, 2: 4.59, 4: 4.09, 8: 3.96 per 100 M lines
#define EM_TILE (256u * EM_ROWS)
__global__ __launch_bounds__(256) void k_paf_emit_chain(PafCols o, const uint32_t *__restrict__ slot_id, uint32_t L, int bi_dir, uint4 *__restrict__ rec, uint32_t *__restrict__ d_total,
                                                         unsigned long long *state, uint32_t *ticket, uint32_t ticket_base, uint32_t epoch)
{
	__shared__ uint32_t s_row[4 * EM_ROWS + 1];
	__shared__ uint32_t s_tile, s_prefix;
	if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u) - ticket_base;
	__syncthreads();
	const uint32_t tile = s_tile;
	const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const size_t tbase = (size_t)tile * EM_TILE;
	uint32_t fl[EM_ROWS], qid[EM_ROWS], tid[EM_ROWS], cnt[EM_ROWS], ex[EM_ROWS];
#pragma unroll
	for (unsigned k = 0; k < EM_ROWS; ++k) {
		const size_t i = tbase + (size_t)(k * 4u + wave) * 64u + lane;
		const bool in = i < L; const size_t j = in ? i : 0;
		fl[k] = in ? o.flags[j] : 0u; qid[k] = o.qslot[j]; tid[k] = o.tslot[j];
	}
#pragma unroll
	for (unsigned k = 0; k < EM_ROWS; ++k) {
		cnt[k] = 0;
		if (fl[k] & 2u) {
			qid[k] = slot_id[qid[k]]; tid[k] = slot_id[tid[k]];
			cnt[k] = 1u + (bi_dir && qid[k] != tid[k]); // hit.c:87-98
		}
		const uint32_t incl = (uint32_t)wv_scan_incl_i32((int)cnt[k], lane);
		ex[k] = incl - cnt[k];
		if (lane == 63) s_row[k * 4u + wave] = incl;
	}
	__syncthreads();
	if (threadIdx.x == 0) { // the rows' totals -> their offsets in the tile, the tile's total
		uint32_t run = 0;
		for (unsigned r = 0; r < 4 * EM_ROWS; ++r) { const uint32_t v = s_row[r]; s_row[r] = run; run += v; }
		s_row[4 * EM_ROWS] = run;
		SC_PUBLISH(&state[tile], sc_pack(epoch, tile == 0 ? SC_INCL : SC_AGG, run));
		if (tile == 0) s_prefix = 0;
	}
	__syncthreads();
	if (tile > 0 && threadIdx.x < 64) {
		const uint32_t tot = s_row[4 * EM_ROWS];
		const uint32_t prefix = sc_look_back(state, tile, epoch, threadIdx.x);
		if (threadIdx.x == 0) { s_prefix = prefix; SC_PUBLISH(&state[tile], sc_pack(epoch, SC_INCL, prefix + tot)); }
	}
	__syncthreads();
	const uint32_t p0 = s_prefix;
#pragma unroll
	for (unsigned k = 0; k < EM_ROWS; ++k) { // (the six number columns are fetched here, a row ahead of its stores: asking for all of them up front bought nothing and costs 6 registers a row)
		if (!cnt[k]) continue;
		const size_t i = tbase + (size_t)(k * 4u + wave) * 64u + lane;
		const uint32_t qs = o.qs[i], qe = o.qe[i], ts = o.ts[i], te = o.te[i];
		const uint32_t mlrev = o.ml[i] | (fl[k] >> 3 & 1u) << 31, b31 = o.bl[i] & 0x7fffffffu;
		uint4 *r = rec + (size_t)(p0 + s_row[k * 4u + wave] + ex[k]) * 2;
		r[0] = make_uint4(qs, qid[k], qe, tid[k]);   // qns = qid<<32 | qs ; qe ; tn
		r[1] = make_uint4(ts, te, mlrev, b31);       // ts ; te ; ml|rev ; bl|del=0
		if (cnt[k] == 2) {
			r[2] = make_uint4(ts, tid[k], te, qid[k]);
			r[3] = make_uint4(qs, qe, mlrev, b31);
		}
	}
	if (threadIdx.x == 0 && tbase < L && tbase + EM_TILE >= L) *d_total = p0 + s_row[4 * EM_ROWS]; // the last tile: its end is the total
}

// ------------------------------------------------------------------------------------------------ host entries

static int paf_reserve_text(mahip_ctx *c, size_t nbytes)
{
	PafBufs *b = paf_of(c);
	{ // a cap on the text the device stage accepts (tests use it to exercise the caller's fall-back to the host reader)
		const char *e = getenv("MA_PAF_MAX_BYTES");
		if (e && nbytes > (size_t)atoll(e)) { mahip_set_error("text of %zu bytes exceeds MA_PAF_MAX_BYTES", nbytes); return -1; }
	}
	const bool timing = ma_timing_level() >= 1;
	struct timespec ts0, ts1;
	if (timing) clock_gettime(CLOCK_MONOTONIC, &ts0);
	CHK(dev_reserve(c, b->text, nbytes + 64));
	if (timing) {
		clock_gettime(CLOCK_MONOTONIC, &ts1);
		fprintf(stderr, "[T::paf] hipMalloc of the text buffer: %.3f s\n", (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec));
	}
	b->nbytes = nbytes;
	b->loaded = false;
	return 0;
}

int paf_text_reserve(mahip_ctx *c, size_t nbytes, void **d_text) { CHK(paf_reserve_text(c, nbytes)); *d_text = paf_of(c)->text.p; return 0; }
void paf_text_loaded(mahip_ctx *c) { paf_of(c)->loaded = true; }

extern "C" int mahip_paf_load_mem(mahip_ctx_t *c, const void *text, size_t nbytes)
{
	HIPCHK(hipSetDevice(c->dev));
	CHK(paf_reserve_text(c, nbytes));
	CHK(xfer_copy(c, paf_of(c)->text.p, (void*)text, nbytes, 1));
	paf_of(c)->loaded = true;
	return 0;
}

extern "C" int mahip_paf_load_fd(mahip_ctx_t *c, int fd, size_t nbytes)
{
	HIPCHK(hipSetDevice(c->dev));
	CHK(paf_reserve_text(c, nbytes));
	CHK(xfer_from_fd(c, paf_of(c)->text.p, fd, nbytes));
	paf_of(c)->loaded = true;
	return 0;
}

extern "C" int mahip_paf_load_fd_range(mahip_ctx_t *c, int fd, size_t off, size_t nbytes)
{ // bytes [off, off + nbytes) of an open plain file: a rank's own range of the text (cut at line starts by the caller)
	HIPCHK(hipSetDevice(c->dev));
	CHK(paf_reserve_text(c, nbytes));
	if (nbytes) CHK(xfer_from_fd_at(c, paf_of(c)->text.p, fd, off, nbytes));
	paf_of(c)->loaded = true;
	return 0;
}

static uint32_t pow2_at_least(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p > 0x80000000ull ? 0x80000000u : (uint32_t)p; }

// a few bytes of device memory, now (the stream is idle afterwards)
static int fetch_bytes(mahip_ctx *c, const void *dptr, void *v, size_t bytes)
{
	HIPCHK(hipMemcpyAsync(v, dptr, bytes, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	return 0;
}
static int fetch_u32(mahip_ctx *c, const void *dptr, uint32_t *v) { return fetch_bytes(c, dptr, v, 4); }

extern "C" int mahip_paf_parse(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, mahip_paf_info_t *info)
{
	return mahip_paf_parse_excl(c, min_span, min_match, bi_dir, 0, 0, 0.f, info);
}

// What the stages of one parse hand each other; lives for one mahip_paf_parse*.  The stages, in the order of this file's header: paf_census, paf_reserve_cols,
// paf_fields, paf_cross_counts (ranks only), paf_stale_bl, paf_dict_local, paf_dict_merged (ranks only), paf_records + paf_adopt.
struct PafParse {
	uint32_t L = 0;           // lines (the virtual newline of an unterminated tail is counted)
	size_t n_eff = 0;         // the tile parser's text: n + the appended newline
	int open_line = 0;
	uint32_t n_gran = 0, tile_k = 1, n_tiles = 0;
	PafCols o;
	size_t n_valid = 0, n_pass = 0, n_nobl = 0, n_long = 0, n_hits = 0;
	uint32_t max_qs = 0, n_excl = 0;
	uint64_t line_base = 0, lines_total = 0, valid_total = 0, pass_total = 0, nobl_total = 0; // lines of the ranges in front of this one; totals over the ranks
	uint32_t R = 0, cap_used = 0; // names with an id; slots of the local table
	int gen_local = 0;            // c->key[gen_local]: the local first appearances, sorted
	const uint32_t *slot_to_id = nullptr; // table slot -> id, for the records
};

// ---- line starts: newline census per KiB, the tile geometry (the tile parser writes the line starts itself)
static int paf_census(mahip_ctx *c, PafBufs *b, PafParse &ps)
{
	const size_t n = b->nbytes;
	const unsigned char *text = P<unsigned char>(b->text);
	CHK(dev_reserve(c, b->scal, 64));
	CHK(ctr_zero(c));
	ps.n_eff = n;
	if (!n) return 0;
	{ // same decision as the kernels': L = newlines + an unterminated tail
		unsigned char last = 0;
		CHK(fetch_bytes(c, text + n - 1, &last, 1));
		ps.open_line = last != '\n';
	}
	// every line ends with a newline: a text that does not gets one (the buffer has 64 spare bytes; the line start after it is n + 1),
	// and zeros follow, so that the kernels read whole 16-byte pieces
	HIPCHK(hipMemsetAsync((void*)(text + n), 0, 64, c->st));
	if (ps.open_line) HIPCHK(hipMemsetAsync((void*)(text + n), '\n', 1, c->st));
	ps.n_eff = n + (size_t)ps.open_line;
	const size_t ng = (ps.n_eff + PAF_GRAN - 1) / PAF_GRAN;
	if (ng > 0x7ffffff0ull) { mahip_set_error("mahip_paf_parse: text too large"); return -1; }
	const uint32_t n_gran = ps.n_gran = (uint32_t)ng;
	CHK(dev_reserve(c, b->tile, ((size_t)n_gran + 8) * 4)); CHK(dev_reserve(c, b->glast, ((size_t)n_gran + 8) * 4));
	{
		ProfScope ps_(c, "k_paf_nl_count", (double)n);
		hipLaunchKernelGGL(k_paf_gran_count, dim3((n_gran + 4 * PAF_GC_PER_WAVE - 1) / (4 * PAF_GC_PER_WAVE)), dim3(256), 0, c->st, text, ps.n_eff, n_gran, P<uint32_t>(b->tile), P<uint32_t>(b->glast));
	}
	CHK(scan_exclusive_u32(c, P<uint32_t>(b->tile), P<uint32_t>(b->tile), n_gran, P<uint32_t>(b->tile) + n_gran)); // goff[n_gran] = all newlines
	uint32_t n_nl = 0;
	CHK(fetch_u32(c, P<uint32_t>(b->tile) + n_gran, &n_nl));
	if ((uint64_t)n_nl + 1 >= 0x7fffffffull) { mahip_set_error("mahip_paf_parse: more than 2^31 lines"); return -1; }
	const uint32_t L = ps.L = n_nl; // (the virtual newline is counted)
	CHK(dev_reserve(c, b->lstart, ((size_t)L + 4) * 8));
	if (!L) return 0;
	// tile = K granules with about 240 lines (a lane per line, 256 lanes); at most what a block stages (15 KiB + 1 KiB in front with 16 KiB of LDS text, 31 + 1 with 32)
	double k = 240.0 * ((double)n / (double)L) / (double)PAF_GRAN;
	if (const char *e = getenv("MA_PAF_TILE_K")) k = atof(e);
	ps.tile_k = k < 1.0 ? 1u : k > 31.0 ? 31u : (uint32_t)k;
	ps.n_tiles = (n_gran + ps.tile_k - 1) / ps.tile_k;
	const uint32_t n_grp = (n_gran >> PAF_BGRP) + 1;
	CHK(dev_reserve(c, b->gmax, ((size_t)n_grp + 1) * 8)); CHK(dev_reserve(c, b->tfirst, ((size_t)ps.n_tiles + 1) * 8));
	hipLaunchKernelGGL(k_paf_gran_bmax, dim3(n_grp), dim3(64), 0, c->st, (const uint32_t*)P<uint32_t>(b->glast), n_gran, P<unsigned long long>(b->gmax));
	hipLaunchKernelGGL(k_paf_tile_first, dim3(grid_for(ps.n_tiles, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(b->glast), (const unsigned long long*)P<unsigned long long>(b->gmax), ps.tile_k, ps.n_tiles,
	                   P<unsigned long long>(b->tfirst));
	return 0;
}

// ---- the per-line columns (and the two work arrays of the passes over them)
static int paf_reserve_cols(mahip_ctx *c, PafBufs *b, PafParse &ps)
{
	PafCols &o = ps.o;
	const size_t Lr = (size_t)ps.L + 4;
	CHK(dev_reserve(c, b->flags, Lr));
	for (int k = 0; k < 8; ++k) CHK(dev_reserve(c, b->num[k], Lr * 4));
	CHK(dev_reserve(c, b->tnoff, Lr * 4)); CHK(dev_reserve(c, b->qlen, Lr * 4)); CHK(dev_reserve(c, b->tlen, Lr * 4));
	CHK(dev_reserve(c, b->hq, Lr * 8)); CHK(dev_reserve(c, b->ht, Lr * 8));
	CHK(dev_reserve(c, b->qslot, Lr * 4)); CHK(dev_reserve(c, b->tslot, Lr * 4));
	o.flags = P<uint8_t>(b->flags);
	o.ql = P<uint32_t>(b->num[0]); o.qs = P<uint32_t>(b->num[1]); o.qe = P<uint32_t>(b->num[2]); o.tl = P<uint32_t>(b->num[3]);
	o.ts = P<uint32_t>(b->num[4]); o.te = P<uint32_t>(b->num[5]); o.ml = P<uint32_t>(b->num[6]); o.bl = P<uint32_t>(b->num[7]);
	o.tnoff = P<uint32_t>(b->tnoff); o.qlen = P<uint32_t>(b->qlen); o.tlen = P<uint32_t>(b->tlen);
	o.hq = P<uint64_t>(b->hq); o.ht = P<uint64_t>(b->ht); o.qslot = P<uint32_t>(b->qslot); o.tslot = P<uint32_t>(b->tslot);
	if (ps.L) { CHK(dev_reserve(c, c->keep, ((size_t)ps.L + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)ps.L + 16) * 4)); }
	return 0;
}

// ---- fields: the tile parser, the byte-wise routine on the lines it left, the counts
static int paf_fields(mahip_ctx *c, PafBufs *b, PafParse &ps, int min_span, int min_match)
{
	const uint32_t L = ps.L;
	if (!L) return 0;
	const unsigned char *text = P<unsigned char>(b->text);
	unsigned long long *ctr = P<unsigned long long>(c->ctr);
	mahip_paf_report_t &rp = b->rep;
	{
		ProfScope ps_(c, "k_paf_parse", (double)b->nbytes + 69.0 * (double)L);
		TileArgs ta;
		ta.text = text; ta.n = ps.n_eff; ta.K = ps.tile_k; ta.n_gran = ps.n_gran; ta.n_tiles = ps.n_tiles; ta.L = L;
		ta.goff = (const uint32_t*)P<uint32_t>(b->tile); ta.first = (const unsigned long long*)P<unsigned long long>(b->tfirst);
		ta.min_span = min_span; ta.min_match = min_match;
		const int ch = ps.tile_k <= 15 ? 1 : 2;
		const uint32_t reg = (uint32_t)ch * 16384u, lds = reg + 32 + 2 * (reg / 16 + 8) * 2 + 260 * 4;
		uint32_t per_cu = (160u * 1024u) / (lds + 64u); if (per_cu > 8) per_cu = 8; // blocks a CU holds: the grid is what fits the chip, a block works through tiles (one set of counter atomics per block)
		const unsigned grid = grid_for(ps.n_tiles, 1, 256u * per_cu);
		rp.tile_form = ch;
		if (ch == 1) hipLaunchKernelGGL(k_paf_parse_tile<1>, dim3(grid), dim3(256), lds, c->st, ta, ps.o, P<uint64_t>(b->lstart), ctr);
		else hipLaunchKernelGGL(k_paf_parse_tile<2>, dim3(grid), dim3(256), lds, c->st, ta, ps.o, P<uint64_t>(b->lstart), ctr);
	}
	CHK(ctr_fetch(c));
	rp.n_odd = c->h_ctr[PC_ODD];
	if (c->paf_keep_odd) { // tests: which lines the tile parser left to the byte-wise routine (the final flags do not say)
		b->odd_snap.resize(L);
		CHK(fetch_bytes(c, ps.o.flags, b->odd_snap.data(), L));
		for (uint8_t &f : b->odd_snap) f = f == PF_ODD;
	}
	if (c->h_ctr[PC_ODD]) { // lines the straight-line parser does not cover: the byte-wise routine on them (the counters add up)
		ProfScope ps_(c, "k_paf_parse_odd", 0.0);
		hipLaunchKernelGGL(k_paf_parse_odd, dim3(grid_for(L, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, text, (const uint64_t*)P<uint64_t>(b->lstart), L, min_span, min_match, ps.o, ctr);
		CHK(ctr_fetch(c));
		rp.odd_ran = 1;
	}
	ps.n_valid = (size_t)c->h_ctr[PC_VALID]; ps.n_pass = (size_t)c->h_ctr[PC_PASS]; ps.n_nobl = (size_t)c->h_ctr[PC_NOBL];
	ps.n_long = (size_t)c->h_ctr[PC_LONG];
	ps.max_qs = (uint32_t)c->h_ctr[PC_MAXQS];
	return 0;
}

// ---- what the ranges have to know of each other before names and records can be numbered (a collective)
static int paf_cross_counts(mahip_ctx *c, PafParse &ps)
{
	const int W = mahip_comm_world(c), me = mahip_comm_rank(c);
	uint64_t mine[5] = { ps.L, ps.n_valid, ps.n_pass, ps.n_nobl, ps.max_qs }, all[5 * 32];
	CHK(mahip_comm_all_gather_u64(c, mine, 5, all));
	for (int r = 0; r < W; ++r) {
		if (r < me) ps.line_base += all[5 * r];
		ps.lines_total += all[5 * r]; ps.valid_total += all[5 * r + 1]; ps.pass_total += all[5 * r + 2]; ps.nobl_total += all[5 * r + 3];
		if (all[5 * r + 4] > ps.max_qs) ps.max_qs = (uint32_t)all[5 * r + 4];
	}
	if (ps.lines_total + 1 >= 0x7fffffffull) { mahip_set_error("mahip_paf_parse_sharded: more than 2^31 lines"); return -1; }
	return 0;
}

// ---- stale bl: rare (PAF writers emit 12+ columns).  The bl of the lines that have one, compacted; a line without takes the one in front of it.
// exchange (a collective: every rank comes here when ANY rank has a 10-column line): every range says what `bl` it leaves behind (the bl of its last 11-column
// line), and a line in front of a range's first 11-column line inherits from the nearest range before it that has one (paf.c:54: the field is simply not written)
// before0 (without the exchange): what the ranges in front of this text leave behind, known to the caller -- the pieces of a stream arrive in order (mahip_paf_stream_piece_mem)
static int paf_stale_bl(mahip_ctx *c, PafBufs *b, PafParse &ps, bool exchange, uint32_t before0 = 0)
{
	const uint32_t L = ps.L;
	uint32_t *has = P<uint32_t>(c->keep), *pos = P<uint32_t>(c->pos);
	uint32_t n_has = 0, last_bl = 0, before = before0;
	if (L) {
		CHK(dev_reserve(c, b->blv, ((size_t)L + 4) * 4));
		hipLaunchKernelGGL(k_paf_hasbl, dim3(grid_for(L, 256)), dim3(256), 0, c->st, (const uint8_t*)ps.o.flags, L, has);
		CHK(scan_exclusive_u32(c, has, pos, L, exchange ? P<uint32_t>(b->scal) : nullptr));
		hipLaunchKernelGGL(k_paf_bl_compact, dim3(grid_for(L, 256)), dim3(256), 0, c->st, (const uint32_t*)has, (const uint32_t*)pos, (const uint32_t*)ps.o.bl, L, P<uint32_t>(b->blv));
		if (exchange) {
			CHK(fetch_u32(c, b->scal.p, &n_has));
			if (n_has) CHK(fetch_u32(c, P<uint32_t>(b->blv) + (n_has - 1), &last_bl));
		}
	}
	if (exchange) {
		const int me = mahip_comm_rank(c);
		uint64_t two[2] = { n_has ? 1u : 0u, last_bl }, every[2 * 32];
		CHK(mahip_comm_all_gather_u64(c, two, 2, every));
		for (int r = 0; r < me; ++r) if (every[2 * r]) before = (uint32_t)every[2 * r + 1];
	}
	if (L && ps.n_nobl) hipLaunchKernelGGL(k_bl_fill_from, dim3(grid_for(L, 256)), dim3(256), 0, c->st, (const uint32_t*)has, (const uint32_t*)pos, (const uint32_t*)P<uint32_t>(b->blv), L, ps.o.bl, before);
	return 0;
}

// A temporary of one stage: its memory goes back when the scope ends, however it ends.  dev_free does not wait and hands the memory to the next buffer that asks, so the
// destructor waits for the stream first: kernels that read the buffer may still be queued when a stage gives up half way
struct ScopedDev {
	mahip_ctx *c;
	DevBuf b;
	explicit ScopedDev(mahip_ctx *c_) : c(c_) {}
	ScopedDev(const ScopedDev&) = delete;
	ScopedDev &operator=(const ScopedDev&) = delete;
	~ScopedDev() { release(); }
	void release() { if (b.p) { (void)hipStreamSynchronize(c->st); dev_free(c, b); } }
};

// lengths + 1 of R names in c->keep -> name_pos and the size of the block; the block; the names copied into it out of `src` (name_off counts from there), a NUL behind
// each.  done_first: a temporary nothing needs any more once the scan is through, released before the block is reserved (the stage's peak memory)
static int paf_name_block(mahip_ctx *c, PafBufs *b, const unsigned char *src, uint32_t R, ScopedDev *done_first = nullptr)
{
	uint32_t nb = 0;
	CHK(scan_exclusive_u32(c, P<uint32_t>(c->keep), P<uint32_t>(b->name_pos), R, P<uint32_t>(b->scal)));
	CHK(fetch_u32(c, b->scal.p, &nb));
	if (done_first) done_first->release();
	CHK(dev_reserve(c, b->names, (size_t)nb + 16));
	if (R) hipLaunchKernelGGL(k_dict_names, dim3(grid_for(R, 256)), dim3(256), 0, c->st, src, (const uint64_t*)P<uint64_t>(b->name_off), (const uint32_t*)P<uint32_t>(b->name_len),
	                          (const uint32_t*)P<uint32_t>(b->name_pos), R, P<char>(b->names));
	b->name_bytes = nb;
	return 0;
}

// ---- dictionary: distinct names, ids in order of first appearance
static int paf_dict_local(mahip_ctx *c, PafBufs *b, PafParse &ps, int no_cont, int max_hang, float int_frac)
{
	const uint32_t L = ps.L;
	const PafCols &o = ps.o;
	const unsigned char *text = P<unsigned char>(b->text);
	unsigned long long *ctr = P<unsigned long long>(c->ctr);
	mahip_paf_report_t &rp = b->rep;
	// The number of distinct names is not known before the pass (<= 2 per stored line; in overlap files a read has tens of lines).  Start with a
	// table sized for 16 lines per name -- 8x smaller than the safe size, it stays in the last-level cache -- count the names as they go in, and
	// repeat the pass with a table for 4x that many only if the load factor came out above 1/2 (or a probe sequence ran out)
	const uint32_t cap_max = pow2_at_least(4 * (uint64_t)ps.n_pass + 65536); // load <= 1/2 whatever the file holds
	uint32_t cap = pow2_at_least(ps.n_pass / 16 + 65536);
	if (const char *e = getenv("MA_DICT_CAP_LOG2")) { int l2 = atoi(e); if (l2 >= 4 && l2 <= 31) cap = 1u << l2; } // tests: force the growth path
	const bool short_names = ps.n_long == 0 && !getenv("MA_DICT_EXACT_TEXT"); // every name is its own key: no text compared (k_dict_insert_short)
	rp.dict_form = short_names ? MAHIP_PAF_DICT_SHORT : MAHIP_PAF_DICT_TEXT;
	for (int attempt = 0;; ++attempt) {
		CHK(dev_reserve(c, b->tab, (size_t)cap * 16)); CHK(dev_reserve(c, b->tmin, (size_t)cap * 4)); CHK(dev_reserve(c, b->slot_id, (size_t)cap * 4));
		CHK(ctr_zero(c));
		if (short_names) {
			HIPCHK(hipMemsetAsync(b->tab.p, 0, (size_t)cap * 16, c->st));
			ProfScope ps_(c, "k_dict_insert", 2.0 * 40.0 * (double)ps.n_pass);
			hipLaunchKernelGGL(k_dict_insert_short, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, o, L, (DSlot*)b->tab.p, cap - 1, ctr);
		} else {
			HIPCHK(hipMemsetAsync(b->tab.p, 0xff, (size_t)cap * 16, c->st));
			ProfScope ps_(c, "k_dict_insert", 2.0 * 40.0 * (double)ps.n_pass);
			hipLaunchKernelGGL(k_dict_insert, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, text, (const uint64_t*)P<uint64_t>(b->lstart), L, o, (XSlot*)b->tab.p, cap - 1, ctr);
		}
		CHK(ctr_fetch(c));
		const uint64_t distinct = c->h_ctr[PC_DISTINCT];
		rp.n_attempts = attempt + 1; rp.cap[attempt] = cap; rp.n_distinct = distinct;
		rp.end[attempt] = c->h_ctr[PC_OVERFLOW] ? MAHIP_PAF_TAB_PROBES : 2 * distinct > cap ? MAHIP_PAF_TAB_LOAD : MAHIP_PAF_TAB_OK;
		if (c->h_ctr[PC_OVERFLOW] == 0 && 2 * distinct <= cap) break;
		if (attempt >= 3 || cap >= cap_max) { if (c->h_ctr[PC_OVERFLOW] == 0) break; mahip_set_error("mahip_paf_parse: name table overflow"); return -1; }
		uint32_t want = pow2_at_least(4 * distinct + 65536);
		if (want <= cap) want = cap < 0x10000000u ? cap << 3 : cap_max; // a probe sequence ran out: the count is incomplete
		cap = want < cap_max ? want : cap_max;
	}
	if (short_names) hipLaunchKernelGGL(k_dict_short_tmin, dim3(grid_for(cap, 256)), dim3(256), 0, c->st, (const DSlot*)b->tab.p, cap, P<uint32_t>(b->tmin));
	else hipLaunchKernelGGL(k_dict_exact_tmin, dim3(grid_for(cap, 256)), dim3(256), 0, c->st, (const XSlot*)b->tab.p, cap, P<uint32_t>(b->tmin));
	if (no_cont) { // hit.c:38-68 + hit.c:86
		CHK(dev_reserve(c, b->excl, (size_t)cap + 16));
		HIPCHK(hipMemsetAsync(b->excl.p, 0, cap, c->st));
		hipLaunchKernelGGL(k_paf_nocont, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, o, L, max_hang, int_frac, P<uint8_t>(b->excl));
		HIPCHK(hipMemsetAsync(b->tmin.p, 0xff, (size_t)cap * 4, c->st));
		CHK(ctr_zero(c));
		hipLaunchKernelGGL(k_paf_refilter, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, o, L, (const uint8_t*)P<uint8_t>(b->excl), P<uint32_t>(b->tmin), ctr);
		hipLaunchKernelGGL(k_excl_count, dim3(grid_for(cap, 256, 2048)), dim3(256), 0, c->st, (const uint8_t*)P<uint8_t>(b->excl), cap, ctr);
		CHK(ctr_fetch(c));
		ps.n_pass = (size_t)c->h_ctr[PC_PASS];
		ps.n_excl = (uint32_t)c->h_ctr[PC_VALID];
	}
	// the slots in use, sorted by first appearance: rank = id
	uint32_t R = 0;
	CHK(dev_reserve(c, c->keep, ((size_t)cap + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)cap + 16) * 4));
	hipLaunchKernelGGL(k_dict_flag, dim3(grid_for(cap, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(b->tmin), cap, P<uint32_t>(c->keep));
	CHK(scan_exclusive_u32(c, P<uint32_t>(c->keep), P<uint32_t>(c->pos), cap, P<uint32_t>(b->scal)));
	CHK(fetch_u32(c, b->scal.p, &R));
	for (int k = 0; k < 2; ++k) { CHK(dev_reserve(c, c->key[k], ((size_t)R + 1) * 8)); CHK(dev_reserve(c, c->val[k], ((size_t)R + 1) * 4)); }
	hipLaunchKernelGGL(k_dict_collect, dim3(grid_for(cap, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(c->keep), (const uint32_t*)P<uint32_t>(c->pos), (const uint32_t*)P<uint32_t>(b->tmin), cap,
	                   P<uint64_t>(c->key[0]), P<uint32_t>(c->val[0]));
	int gen = 0;
	CHK(radix_sort_pairs(c, R, 0, bitlen_u64(2ull * L), 0, 0, &gen));
	CHK(dev_reserve(c, b->seq_len, ((size_t)R + 4) * 4)); CHK(dev_reserve(c, b->name_off, ((size_t)R + 4) * 8));
	CHK(dev_reserve(c, b->name_len, ((size_t)R + 4) * 4)); CHK(dev_reserve(c, b->name_pos, ((size_t)R + 4) * 4));
	hipLaunchKernelGGL(k_dict_assign, dim3(grid_for(R, 256)), dim3(256), 0, c->st, (const uint64_t*)P<uint64_t>(c->key[gen]), (const uint32_t*)P<uint32_t>(c->val[gen]), R,
	                   (const uint64_t*)P<uint64_t>(b->lstart), o, P<uint32_t>(b->slot_id), P<uint32_t>(b->seq_len), P<uint64_t>(b->name_off), P<uint32_t>(b->name_len), P<uint32_t>(c->keep));
	CHK(paf_name_block(c, b, text, R));
	ps.R = R; ps.cap_used = cap; ps.gen_local = gen;
	return 0;
}

// ---- the ranks' name tables -> one dictionary (kernels above; a collective)
static int paf_dict_merged(mahip_ctx *c, PafBufs *b, PafParse &ps)
{
	const int W = mahip_comm_world(c), me = mahip_comm_rank(c);
	unsigned long long *ctr = P<unsigned long long>(c->ctr);
	const uint32_t R_loc = ps.R, cap_used = ps.cap_used;
	const size_t nb_loc = b->name_bytes;
	uint64_t mine[2] = { R_loc, nb_loc }, all[2 * 32];
	CHK(mahip_comm_all_gather_u64(c, mine, 2, all));
	uint32_t stride_rows = 1, h_rows[32];
	size_t stride_bytes = 16, sum_rows = 0;
	for (int r = 0; r < W; ++r) { h_rows[r] = (uint32_t)all[2 * r]; sum_rows += all[2 * r]; if (all[2 * r] > stride_rows) stride_rows = (uint32_t)all[2 * r]; if (all[2 * r + 1] > stride_bytes) stride_bytes = (size_t)all[2 * r + 1]; }
	stride_bytes = (stride_bytes + 15) & ~(size_t)15;
	if ((uint64_t)stride_rows * (uint64_t)W >= 0xffffffffull) { mahip_set_error("mahip_paf_parse_sharded: too many names"); return -1; }
	// my rows and name bytes into exchange buffers, gathered with the stride of the largest range
	ScopedDev rows_all(c), blobs_all(c), aux(c);
	void *xr = nullptr, *xb = nullptr;
	CHK(mahip_xbuf(c, 0, (size_t)stride_rows * sizeof(NameRow) + stride_bytes, &xr));
	xb = (char*)xr + (size_t)stride_rows * sizeof(NameRow);
	if (R_loc) {
		hipLaunchKernelGGL(k_name_rows, dim3(grid_for(R_loc, 256)), dim3(256), 0, c->st, (const uint64_t*)P<uint64_t>(c->key[ps.gen_local]), R_loc, (uint32_t)(2 * ps.line_base), (const uint32_t*)P<uint32_t>(b->seq_len),
		                   (const uint32_t*)P<uint32_t>(b->name_len), (const uint32_t*)P<uint32_t>(b->name_pos), (NameRow*)xr);
		HIPCHK(hipMemcpyAsync(xb, b->names.p, nb_loc, hipMemcpyDeviceToDevice, c->st));
	}
	CHK(dev_reserve(c, rows_all.b, (size_t)W * stride_rows * sizeof(NameRow) + 64));
	CHK(dev_reserve(c, blobs_all.b, (size_t)W * stride_bytes + 64));
	CHK(mahip_comm_all_gather(c, xr, rows_all.b.p, (size_t)stride_rows * sizeof(NameRow)));
	CHK(mahip_comm_all_gather(c, xb, blobs_all.b.p, stride_bytes));
	// one table for all of them: at most sum_rows distinct names
	const uint32_t gcap = pow2_at_least(2 * (uint64_t)sum_rows + 1024);
	const size_t total_rows = (size_t)W * stride_rows;
	// aux: tab[gcap] u64 | gkey[gcap] u64 | slot_of[total_rows] u32 | gid_of_slot[gcap] u32 | n_rows[32] u32
	const size_t o_key = (size_t)gcap * 8, o_slot = o_key + (size_t)gcap * 8, o_gid = o_slot + ((total_rows * 4 + 7) & ~(size_t)7), o_n = o_gid + (size_t)gcap * 4;
	CHK(dev_reserve(c, aux.b, o_n + 32 * 4 + 64));
	char *const ax = (char*)aux.b.p;
	unsigned long long *gtab = (unsigned long long*)ax, *gkey = (unsigned long long*)(ax + o_key);
	uint32_t *slot_of = (uint32_t*)(ax + o_slot), *gid_of_slot = (uint32_t*)(ax + o_gid), *d_rows = (uint32_t*)(ax + o_n);
	HIPCHK(hipMemsetAsync(ax, 0xff, o_slot, c->st));
	HIPCHK(hipMemcpyAsync(d_rows, h_rows, (size_t)W * 4, hipMemcpyHostToDevice, c->st));
	CHK(ctr_zero(c));
	if (sum_rows) hipLaunchKernelGGL(k_dict_merge, dim3(grid_for(total_rows, 256, 8192)), dim3(256), 0, c->st, (const NameRow*)rows_all.b.p, (const unsigned char*)blobs_all.b.p, (const uint32_t*)d_rows, W,
	                                 stride_rows, stride_bytes, gtab, gkey, gcap - 1, slot_of, ctr);
	CHK(ctr_fetch(c));
	if (c->h_ctr[PC_OVERFLOW]) { mahip_set_error("mahip_paf_parse_sharded: name table overflow"); return -1; }
	// distinct names sorted by first appearance = ids
	CHK(dev_reserve(c, c->keep, ((size_t)gcap + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)gcap + 16) * 4));
	hipLaunchKernelGGL(k_merge_flag, dim3(grid_for(gcap, 256)), dim3(256), 0, c->st, (const unsigned long long*)gtab, gcap, P<uint32_t>(c->keep));
	CHK(scan_exclusive_u32(c, P<uint32_t>(c->keep), P<uint32_t>(c->pos), gcap, P<uint32_t>(b->scal)));
	uint32_t Rg = 0;
	CHK(fetch_u32(c, b->scal.p, &Rg));
	for (int k = 0; k < 2; ++k) { CHK(dev_reserve(c, c->key[k], ((size_t)Rg + 1) * 8)); CHK(dev_reserve(c, c->val[k], ((size_t)Rg + 1) * 4)); }
	hipLaunchKernelGGL(k_merge_collect, dim3(grid_for(gcap, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(c->keep), (const uint32_t*)P<uint32_t>(c->pos), (const unsigned long long*)gkey, gcap,
	                   P<uint64_t>(c->key[0]), P<uint32_t>(c->val[0]));
	int gen = 0;
	CHK(radix_sort_pairs(c, Rg, 0, bitlen_u64(2ull * ps.lines_total), 0, 0, &gen));
	// the map for this rank's records BEFORE the local arrays are overwritten: local slot -> global id (k_merge_map needs the local "slot in use" flags)
	if (cap_used) CHK(dev_reserve(c, b->excl, (size_t)cap_used * 4 + 16)); // (the -R flag array is free in this mode: the map lives there)
	CHK(dev_reserve(c, b->seq_len, ((size_t)Rg + 4) * 4)); CHK(dev_reserve(c, b->name_off, ((size_t)Rg + 4) * 8));
	CHK(dev_reserve(c, b->name_len, ((size_t)Rg + 4) * 4)); CHK(dev_reserve(c, b->name_pos, ((size_t)Rg + 4) * 4));
	// keep / pos are about to be reused for the name lengths: the local flags first
	ScopedDev used_local(c);
	if (cap_used) {
		CHK(dev_reserve(c, used_local.b, (size_t)cap_used * 4 + 16));
		hipLaunchKernelGGL(k_dict_flag, dim3(grid_for(cap_used, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(b->tmin), cap_used, (uint32_t*)used_local.b.p);
	}
	CHK(dev_reserve(c, c->keep, ((size_t)Rg + 16) * 4));
	if (Rg) hipLaunchKernelGGL(k_merge_assign, dim3(grid_for(Rg, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(c->val[gen]), Rg, (const unsigned long long*)gtab, (const unsigned long long*)gkey,
	                           (const NameRow*)rows_all.b.p, stride_rows, stride_bytes, gid_of_slot, P<uint32_t>(b->seq_len), P<uint64_t>(b->name_off), P<uint32_t>(b->name_len), P<uint32_t>(c->keep));
	if (cap_used) hipLaunchKernelGGL(k_merge_map, dim3(grid_for(cap_used, 256)), dim3(256), 0, c->st, (const uint32_t*)used_local.b.p, (const uint32_t*)P<uint32_t>(b->slot_id), cap_used,
	                                 (const uint32_t*)slot_of, (uint32_t)((size_t)me * stride_rows), (const uint32_t*)gid_of_slot, P<uint32_t>(b->excl));
	CHK(paf_name_block(c, b, (const unsigned char*)blobs_all.b.p, Rg, &used_local));
	ps.R = Rg; b->n_seq = Rg;
	ps.slot_to_id = (const uint32_t*)P<uint32_t>(b->excl);
	return 0; // (the gathered blocks are released here: their guards wait for k_dict_names)
}

// ---- records: hit (+ mirrored hit) per stored line, in line order.  One pass: ids, record slots (chained tiles), records
// dst: where the records go -- nullptr: the context's own record buffer, sized here; a streamed ingest hands in the place behind the records of the pieces so far
static int paf_records(mahip_ctx *c, PafBufs *b, PafParse &ps, int bi_dir, ma_hit_t *dst = nullptr)
{
	const size_t max_hits = bi_dir ? 2 * ps.n_pass : ps.n_pass;
	if (max_hits >= 0xffffffffull) { mahip_set_error("mahip_paf_parse: more than 2^32 records"); return -1; }
	if (!dst) { CHK(dev_reserve(c, c->aos_own, (max_hits + 1) * sizeof(ma_hit_t))); dst = (ma_hit_t*)c->aos_own.p; }
	const size_t nb = ((size_t)ps.L + EM_TILE - 1) / EM_TILE;
	uint32_t *ticket; unsigned long long *state; uint32_t ticket_base, epoch;
	CHK(scan_chain_begin(c, nb, &state, &ticket, &ticket_base, &epoch));
	uint32_t nh = 0;
	{
		ProfScope ps_(c, "k_paf_emit", 37.0 * (double)ps.n_pass + 32.0 * (double)max_hits);
		hipLaunchKernelGGL(k_paf_emit_chain, dim3((unsigned)nb), dim3(256), 0, c->st, ps.o, ps.slot_to_id, ps.L, bi_dir, (uint4*)dst, P<uint32_t>(b->scal), state, ticket, ticket_base, epoch);
	}
	CHK(fetch_u32(c, b->scal.p, &nh));
	ps.n_hits = nh;
	return 0;
}
// the context takes the records as its input (none: a one-record buffer, so that d_aos points somewhere)
static int paf_adopt(mahip_ctx *c, PafParse &ps)
{
	CHK(mahip_hits_adopt(c, nullptr, ps.n_hits, ps.R)); // resets the per-upload state and sizes the read arrays
	CHK(dev_reserve(c, c->aos_own, sizeof(ma_hit_t)));
	c->d_aos = (const ma_hit_t*)c->aos_own.p;
	return 0;
}

// sharded: the text in the context is THIS RANK'S byte range of the file (cut at line starts, ranges in rank order); the context has a communicator.  The ranks
// exchange what the sequential semantics need across range borders -- line counts (occurrence numbers count lines of the whole file), the last `bl` a range
// leaves behind, the distinct names of every range with their first appearances -- and every rank ends with the records of ITS lines carrying the ids the
// reference would give (the same dictionary on every rank).  info: n_lines / n_records / n_stored_lines are totals over the ranks, n_hits is this rank's.
static int paf_parse_impl(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, int no_cont, int max_hang, float int_frac, mahip_paf_info_t *info, bool sharded)
{
	HIPCHK(hipSetDevice(c->dev));
	PafBufs *b = paf_of(c);
	if (sharded && no_cont) { mahip_set_error("mahip_paf_parse_sharded: the -R pre-filter needs the whole text on one rank"); return -1; }
	if (sharded && mahip_comm_world(c) > 32) { mahip_set_error("mahip_paf_parse_sharded: at most 32 ranks"); return -1; }
	if (!b->loaded) { mahip_set_error("mahip_paf_parse: no text loaded"); return -1; }
	memset(info, 0, sizeof(*info));
	b->n_seq = 0; b->name_bytes = 0;
	b->parsed = false; b->rep = {}; b->odd_snap.clear();
	mahip_paf_report_t &rp = b->rep;
	// MA_PIPE_TIMING=2: wall-clock laps of this function's parts on stderr (each lap waits for the stream: a diagnostic, it changes what it measures by the waits)
	const bool laps = ma_timing_level() >= 2;
	struct timespec lap_t0;
	if (laps) clock_gettime(CLOCK_MONOTONIC, &lap_t0);
	auto lap = [&](const char *what) {
		if (!laps) return;
		(void)hipStreamSynchronize(c->st);
		struct timespec t1;
		clock_gettime(CLOCK_MONOTONIC, &t1);
		fprintf(stderr, "[T::paf_parse] %-28s %9.3f ms\n", what, ((double)(t1.tv_sec - lap_t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - lap_t0.tv_nsec)) * 1e3);
		lap_t0 = t1;
	};
	PafParse ps;
	CHK(paf_census(c, b, ps));
	lap("line census");
	CHK(paf_reserve_cols(c, b, ps));
	if (ps.L) lap("columns reserved");
	CHK(paf_fields(c, b, ps, min_span, min_match));
	if (!sharded && ps.n_nobl) { rp.bl_pass = 1; CHK(paf_stale_bl(c, b, ps, false)); }
	rp.n_lines = ps.L; rp.n_gran = ps.n_gran; rp.tile_k = ps.tile_k; rp.n_tiles = ps.n_tiles; rp.open_line = ps.open_line; rp.n_long = ps.n_long;
	lap("fields");
	if (sharded) {
		CHK(paf_cross_counts(c, ps));
		if (ps.nobl_total) CHK(paf_stale_bl(c, b, ps, true));
	}
	if (ps.n_pass) CHK(paf_dict_local(c, b, ps, no_cont, max_hang, int_frac));
	b->n_seq = ps.R;
	lap("dictionary");
	ps.slot_to_id = P<uint32_t>(b->slot_id);
	if (sharded) CHK(paf_dict_merged(c, b, ps));
	if (ps.n_pass) { CHK(paf_records(c, b, ps, bi_dir)); lap("records"); }
	CHK(paf_adopt(c, ps));
	if (ps.n_pass) lap("adopt");
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->st));
	c->hint_max_qs = c->paf_max_qs = ps.max_qs;
	rp.n_excl = info->n_excl = ps.n_excl;
	b->parsed = true;
	c->run_stride = sharded ? 0 : bi_dir ? 2 : 1; // k_paf_emit_chain wrote a line's record and its mirror side by side (hit.c:87-98): the sort may take RUNS of records (hits.hip)
	info->n_records = ps.n_valid; info->n_stored_lines = ps.n_pass; info->n_hits = ps.n_hits; info->n_seq = ps.R; info->max_qs = ps.max_qs; info->name_bytes = b->name_bytes; info->n_lines = ps.L;
	if (sharded) { info->n_records = ps.valid_total; info->n_stored_lines = ps.pass_total; info->n_lines = ps.lines_total; }
	return 0;
}

extern "C" int mahip_paf_parse_excl(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, int no_cont, int max_hang, float int_frac, mahip_paf_info_t *info)
{
	return paf_parse_impl(c, min_span, min_match, bi_dir, no_cont, max_hang, int_frac, info, false);
}
extern "C" int mahip_paf_parse_sharded(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, mahip_paf_info_t *info)
{
	return paf_parse_impl(c, min_span, min_match, bi_dir, 0, 0, 0.f, info, mahip_comm_active(c) != 0);
}

// ------------------------------------------------------------------------------------------------ streamed ingest: pieces of one text, in order
// The pieces of a stream are ranks in time (the sharded ingest above joins ranges of one text the same way), with one simplification: they arrive in order, so
// a name that is new in piece k takes the ids behind those of all earlier pieces (sdict.c:27-45: ids in order of first appearance) and no sort over the first
// appearances of the whole text is needed.  What persists between pieces: a table of the names so far (open addressing, one 64-bit word per slot:
// tag(32) | id), the names themselves in an arena laid out as mahip_paf_names hands them out (NUL behind each, id order), their first-seen lengths, the records
// so far, the `bl` of the last line with an 11th column (paf.c:54), and the running totals.  A piece runs the stages of a whole parse on its own text; its local
// dictionary (distinct names in local first-appearance order) is then FOLDED into the table: found names keep their id and length, the others get
// n_seq + their rank among the piece's new names -- local ids rise with 2 x line + column, so the order is the reference's.
#define ST_PROV 0x80000000u // low word of a slot claimed in the fold that is running: ST_PROV | local id (ids stay below 2^31); made an id by k_stream_commit

struct PafStream {
	bool active = false, closed = false; // between begin and end / abort; the last piece has been seen
	int min_span = 0, min_match = 0, bi_dir = 0;
	DevBuf tab, arena, seq_len, name_pos, name_len, rec, fold, map;
	uint32_t cap = 0, n_seq = 0;
	size_t arena_bytes = 0, n_rec = 0, rec_cap = 0;
	uint64_t n_lines = 0, n_valid = 0, n_pass = 0;
	uint32_t max_qs = 0, last_bl = 0;
	bool have_bl = false, any_parsed = false;
	mahip_paf_stream_report_t rep = {};
	// -R in the stream (mahip_paf_stream_begin_excl; none of it exists without no_cont): a byte per provisional id, 1 = clearly contained (hit.c:38-68); per record, the
	// lengths of its two names (ql, tl; a mirror record holds them swapped) -- what the first-seen length of a read is taken from once it is known which lines survive
	int no_cont = 0, max_hang = 0, early = 1;
	float int_frac = 0.f;
	DevBuf excl, lens;
	mahip_paf_stream_excl_report_t xrep = {};
};

static void paf_stream_free(mahip_ctx *c, PafBufs *b)
{
	PafStream *st = b->stream;
	if (!st) return;
	DevBuf *all[] = { &st->tab, &st->arena, &st->seq_len, &st->name_pos, &st->name_len, &st->rec, &st->fold, &st->map, &st->excl, &st->lens };
	for (DevBuf *d : all) dev_free(c, *d);
	delete st;
	b->stream = nullptr;
}

// the hash that places a name in the persistent table: over the bytes alone, so that a piece of short names and a piece of long ones meet in one table
__device__ __forceinline__ uint64_t stream_hash(const unsigned char *__restrict__ nm, uint32_t len) { return key_mix(fnv_bytes(nm, len)); }

// One thread per local name j (names of one piece are distinct: two threads never look for the same name).  Found: l2g[j] = its id, is_new[j] = 0.  Not found: the
// first free slot of its probe sequence is claimed (CAS) with ST_PROV | j, slot_of[j] says which, is_new[j] = 1, blen[j] = its bytes in the arena.  A slot that
// holds another thread's claim holds another name: the probe goes on.  At most PAF_PROBE_LIMIT probes; a sequence that runs out raises PC_OVERFLOW (the host
// rebuilds a larger table from the arena, which drops every claim of this launch, and repeats the fold).
__global__ __launch_bounds__(256) void k_stream_fold(const unsigned char *__restrict__ lnames, const uint32_t *__restrict__ lpos, const uint32_t *__restrict__ llen, uint32_t R,
                                                      unsigned long long *__restrict__ tab, uint32_t mask, const unsigned char *__restrict__ arena, const uint32_t *__restrict__ g_pos,
                                                      const uint32_t *__restrict__ g_len, uint32_t *__restrict__ l2g, uint32_t *__restrict__ slot_of, uint32_t *__restrict__ is_new,
                                                      uint32_t *__restrict__ blen, unsigned long long *__restrict__ ctr)
{
	uint32_t fail = 0;
	for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < R; j += gridDim.x * 256u) {
		const uint32_t len = llen[j];
		const unsigned char *nm = lnames + lpos[j];
		const uint64_t h = stream_hash(nm, len);
		const uint32_t tag = (uint32_t)(h >> 32);
		uint32_t s = (uint32_t)h & mask, found = 0xffffffffu, claimed = 0xffffffffu;
		for (uint32_t probe = 0; probe < PAF_PROBE_LIMIT; ++probe, s = (s + 1) & mask) {
			unsigned long long e = tab[s];
			if (e == PAF_EMPTY) {
				e = atomicCAS(&tab[s], PAF_EMPTY, (unsigned long long)tag << 32 | (ST_PROV | j));
				if (e == PAF_EMPTY) { claimed = s; break; }
			}
			const uint32_t v = (uint32_t)e;
			if ((uint32_t)(e >> 32) == tag && !(v & ST_PROV) && g_len[v] == len && name_eq(nm, arena + g_pos[v], len)) { found = v; break; } // the bytes decide, never the tag alone
		}
		is_new[j] = claimed != 0xffffffffu;
		blen[j] = claimed != 0xffffffffu ? len + 1u : 0u;
		slot_of[j] = claimed;
		l2g[j] = found;
		if (found == 0xffffffffu && claimed == 0xffffffffu) fail = 1;
	}
	blk_add_u64(&ctr[PC_OVERFLOW], fail);
}
// the new names get their ids (n_seq0 + rank among the piece's new names, in local-id order) and their places: slot, arena (bytes + NUL at arena0 + bpos[j] .. < arena0 +
// the scanned total), first-seen length.  One thread per local name; every write goes to an index the scans made unique.
__global__ __launch_bounds__(256) void k_stream_commit(const unsigned char *__restrict__ lnames, const uint32_t *__restrict__ lpos, const uint32_t *__restrict__ llen,
                                                        const uint32_t *__restrict__ lseq, uint32_t R, const uint32_t *__restrict__ is_new, const uint32_t *__restrict__ pos,
                                                        const uint32_t *__restrict__ bpos, const uint32_t *__restrict__ slot_of, uint32_t n_seq0, uint32_t arena0,
                                                        unsigned long long *__restrict__ tab, unsigned char *__restrict__ arena, uint32_t *__restrict__ g_pos, uint32_t *__restrict__ g_len,
                                                        uint32_t *__restrict__ g_seq, uint32_t *__restrict__ l2g)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= R || !is_new[j]) return;
	const uint32_t g = n_seq0 + pos[j], len = llen[j], at = arena0 + bpos[j];
	const unsigned char *nm = lnames + lpos[j];
	tab[slot_of[j]] = (tab[slot_of[j]] & 0xffffffff00000000ull) | g; // (the claim is this thread's own: nobody else writes the slot)
	for (uint32_t k = 0; k < len; ++k) arena[at + k] = nm[k];
	arena[at + len] = 0;
	g_pos[g] = at; g_len[g] = len; g_seq[g] = lseq[j];
	l2g[j] = g;
}
// the piece's table slot -> global id, through the slot's local id: what k_merge_map makes for a rank (k_paf_emit_chain's slot_id)
__global__ __launch_bounds__(256) void k_stream_map(const uint32_t *__restrict__ tmin, const uint32_t *__restrict__ slot_id, uint32_t cap, const uint32_t *__restrict__ l2g, uint32_t *__restrict__ out)
{
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s < cap && tmin[s] != 0xffffffffu) out[s] = l2g[slot_id[s]];
}
// a fresh (all PAF_EMPTY) table from the arena: one thread per id so far, exactly those ids are inserted; all names differ, so nothing is compared
__global__ __launch_bounds__(256) void k_stream_rebuild(const unsigned char *__restrict__ arena, const uint32_t *__restrict__ g_pos, const uint32_t *__restrict__ g_len, uint32_t n_seq,
                                                         unsigned long long *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ ctr)
{
	uint32_t fail = 0;
	for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < n_seq; g += gridDim.x * 256u) {
		const uint64_t h = stream_hash(arena + g_pos[g], g_len[g]);
		uint32_t s = (uint32_t)h & mask, probe = 0;
		for (; probe < PAF_PROBE_LIMIT; ++probe, s = (s + 1) & mask)
			if (tab[s] == PAF_EMPTY && atomicCAS(&tab[s], PAF_EMPTY, (unsigned long long)((h >> 32) << 32 | g)) == PAF_EMPTY) break;
		if (probe == PAF_PROBE_LIMIT) fail = 1;
	}
	blk_add_u64(&ctr[PC_OVERFLOW], fail);
}
// what a piece leaves behind for the 10-column lines of later pieces: out[0] = it has a line with an 11th column, out[1] = the bl of the last such line;
// out[2] = the flags of its first line.  One wave walks back from the last line, 64 lines a step, at most ceil(L / 64) steps.
__global__ __launch_bounds__(64) void k_stream_last_bl(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ bl, uint32_t L, uint32_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x;
	uint32_t has = 0, v = 0;
	for (long top = (long)L; top > 0 && !has; top -= 64) {
		const long i = top - 1 - (long)lane;
		const bool mine = i >= 0 && (flags[i] & 4u);
		const unsigned long long m = __ballot(mine);
		if (m) { const int src = __ffsll((long long)m) - 1; v = wv_bcast(mine ? bl[i] : 0u, src); has = 1; } // the lowest lane holds the highest line
	}
	if (lane == 0) { out[0] = has; out[1] = v; out[2] = flags[0]; }
}

// ---- -R in the stream.  The exclusion is a property of NAMES (k_paf_nocont above), and a name keeps its provisional id for the whole stream, so the
// flag lives per provisional id and only ever goes from 0 to 1.  Per piece, behind the fold (map: the piece's table slot -> provisional id, every slot of a stored
// line has one): every stored line gives its verdict, then the stored lines that touch a flagged id -- flagged now or by any earlier piece -- lose their stored
// bit.  A line that is kept here may still die at the end, by a flag a later piece raises (k_stream_mark).
__global__ __launch_bounds__(256) void k_stream_verdict(PafCols o, uint32_t L, const uint32_t *__restrict__ map, int max_hang, float int_frac, uint8_t *__restrict__ excl)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < L; i += gridDim.x * 256u) {
		if (!(o.flags[i] & 2)) continue;
		const int v = mc_no_cont(o.ql[i], o.qs[i], o.qe[i], o.tl[i], o.ts[i], o.te[i], o.flags[i] >> 3 & 1, max_hang, int_frac);
		if (v == 1) excl[map[o.tslot[i]]] = 1;
		else if (v == 2) excl[map[o.qslot[i]]] = 1;
	}
}
// drop != 0: the early drop.  cnt[i] = the records line i will give (k_paf_emit_chain: 1, or 2 with bi_dir and two different names; 0 when it is not stored)
__global__ __launch_bounds__(256) void k_stream_early(PafCols o, uint32_t L, const uint32_t *__restrict__ map, const uint8_t *__restrict__ excl, int drop, int bi_dir,
                                                       uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr)
{
	uint32_t pass = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < L; i += gridDim.x * 256u) {
		uint32_t n = 0;
		if (o.flags[i] & 2) {
			const uint32_t q = map[o.qslot[i]], t = map[o.tslot[i]];
			if (drop && (excl[q] || excl[t])) o.flags[i] &= (uint8_t)~2u;
			else { n = 1u + (bi_dir && q != t); ++pass; }
		}
		cnt[i] = n;
	}
	blk_add_u64(&ctr[PC_PASS], pass);
}
// the lengths column of the piece's records: pos = the exclusive scan of cnt, which is where k_paf_emit_chain puts line i's record (lens: the place of the piece's first)
__global__ __launch_bounds__(256) void k_stream_lens(PafCols o, uint32_t L, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pos, uint2 *__restrict__ lens)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < L; i += gridDim.x * 256u) {
		const uint32_t n = cnt[i];
		if (!n) continue;
		const uint32_t ql = o.ql[i], tl = o.tl[i];
		lens[pos[i]] = make_uint2(ql, tl);
		if (n == 2) lens[pos[i] + 1u] = make_uint2(tl, ql);
	}
}
// At the end.  A record dies when either of its ids is flagged (both records of a -b line carry the same two ids: they die together).  A surviving record r
// brings its two names' first appearance down to 2r (query) and 2r + 1 (target): records are in line order and a mirror sits behind its twin, so the order of
// these minima is the order of first appearance among the surviving lines (hit.c:86-90).  alive[r] = 1 / 0; counted: surviving records, and of them self hits
// (one record per line even with bi_dir: what the line count is made of).
__global__ __launch_bounds__(256) void k_stream_mark(const uint4 *__restrict__ rec, size_t n_rec, const uint8_t *__restrict__ excl, unsigned long long *__restrict__ first,
                                                      uint32_t *__restrict__ alive, unsigned long long *__restrict__ ctr)
{
	uint32_t n_alive = 0, n_self = 0;
	for (size_t r = (size_t)blockIdx.x * 256u + threadIdx.x; r < n_rec; r += (size_t)gridDim.x * 256u) {
		const uint4 a = rec[2 * r];
		const uint32_t q = a.y, t = a.w, ok = !(excl[q] || excl[t]);
		alive[r] = ok;
		if (!ok) continue;
		atomicMin(&first[q], (unsigned long long)(2 * r)); atomicMin(&first[t], (unsigned long long)(2 * r + 1));
		++n_alive; n_self += q == t;
	}
	blk_add_u64(&ctr[PC_PASS], n_alive);
	blk_add_u64(&ctr[PC_VALID], n_self);
}
__global__ __launch_bounds__(256) void k_stream_id_flag(const unsigned long long *__restrict__ first, uint32_t n_seq, uint32_t *__restrict__ keep)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x;
	if (g < n_seq) keep[g] = first[g] != PAF_EMPTY;
}
__global__ __launch_bounds__(256) void k_stream_id_collect(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, const unsigned long long *__restrict__ first, uint32_t n_seq,
                                                            uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x;
	if (g < n_seq && keep[g]) { key[pos[g]] = first[g]; val[pos[g]] = g; }
}
// the survivors sorted by first appearance: rank = the new id (sdict.c:27-45).  Its first-seen length is the one of that appearance (the lengths column), which
// is what k_dict_assign takes in a whole parse; blen[j] = its bytes in the new arena
__global__ __launch_bounds__(256) void k_stream_id_assign(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t R, const uint32_t *__restrict__ old_len,
                                                           const uint2 *__restrict__ lens, uint32_t *__restrict__ new_id, uint32_t *__restrict__ name_len, uint32_t *__restrict__ seq_len,
                                                           uint32_t *__restrict__ blen)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= R) return;
	const uint32_t g = val[j], len = old_len[g];
	const uint64_t occ = key[j];
	const uint2 l = lens[occ >> 1];
	new_id[g] = j;
	name_len[j] = len;
	seq_len[j] = occ & 1 ? l.y : l.x;
	blen[j] = len + 1u;
}
__global__ __launch_bounds__(256) void k_stream_names(const unsigned char *__restrict__ arena, const uint32_t *__restrict__ old_pos, const uint32_t *__restrict__ val,
                                                       const uint32_t *__restrict__ name_pos, const uint32_t *__restrict__ name_len, uint32_t R, unsigned char *__restrict__ out)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= R) return;
	const unsigned char *s = arena + old_pos[val[j]];
	unsigned char *d = out + name_pos[j];
	const uint32_t len = name_len[j];
	for (uint32_t k = 0; k < len; ++k) d[k] = s[k];
	d[len] = 0;
}
// the surviving records, in order, with both ids relabelled (pos: the exclusive scan of alive, in the same array; a survivor's ids have a new id)
__global__ __launch_bounds__(256) void k_stream_compact(const uint4 *__restrict__ rec, size_t n_rec, const uint8_t *__restrict__ excl, const uint32_t *__restrict__ pos,
                                                         const uint32_t *__restrict__ new_id, uint4 *__restrict__ out)
{
	for (size_t r = (size_t)blockIdx.x * 256u + threadIdx.x; r < n_rec; r += (size_t)gridDim.x * 256u) {
		uint4 a = rec[2 * r];
		if (excl[a.y] || excl[a.w]) continue;
		a.y = new_id[a.y]; a.w = new_id[a.w];
		out[2 * (size_t)pos[r]] = a;
		out[2 * (size_t)pos[r] + 1] = rec[2 * r + 1];
	}
}

// a persistent buffer that must hold `need` bytes and keep its first `used`: a new one (at least twice the old) and a device-to-device copy
static int stream_grow(mahip_ctx *c, DevBuf &b, size_t used, size_t need, int *grown = nullptr)
{
	if (need <= b.cap) return 0;
	DevBuf nb;
	CHK(dev_reserve(c, nb, need > 2 * b.cap ? need : 2 * b.cap));
	if (used) HIPCHK(hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, c->st));
	HIPCHK(hipStreamSynchronize(c->st)); // dev_free hands the old memory on at once
	if (grown && b.p) *grown = 1; // (the first buffer replaces none)
	dev_free(c, b);
	b = nb;
	return 0;
}

static int stream_table(mahip_ctx *c, PafStream *st, uint32_t cap)
{ // a table of `cap` slots holding the names so far; a probe sequence that runs out: four times the slots
	for (;; cap = cap < 0x40000000u ? cap << 2 : 0x80000000u) {
		CHK(dev_reserve(c, st->tab, (size_t)cap * 8));
		HIPCHK(hipMemsetAsync(st->tab.p, 0xff, (size_t)cap * 8, c->st));
		CHK(ctr_zero(c));
		if (st->n_seq) hipLaunchKernelGGL(k_stream_rebuild, dim3(grid_for(st->n_seq, 256, 8192)), dim3(256), 0, c->st, (const unsigned char*)P<unsigned char>(st->arena), (const uint32_t*)P<uint32_t>(st->name_pos),
		                                  (const uint32_t*)P<uint32_t>(st->name_len), st->n_seq, P<unsigned long long>(st->tab), cap - 1, P<unsigned long long>(c->ctr));
		CHK(ctr_fetch(c));
		if (st->cap) ++st->rep.n_rebuilds; // (the first table replaces none)
		st->cap = cap;
		if (c->h_ctr[PC_OVERFLOW] == 0) return 0;
		if (cap >= 0x80000000u) { mahip_set_error("mahip_paf_stream_piece_mem: name table overflow"); return -1; }
	}
}

// the fold: the piece's local dictionary (paf_dict_local: b->names / name_pos / name_len / seq_len, R names in local first-appearance order) into the persistent one
static int paf_stream_fold(mahip_ctx *c, PafBufs *b, PafStream *st, PafParse &ps)
{
	const uint32_t R = ps.R;
	mahip_paf_stream_report_t &sr = st->rep;
	if ((uint64_t)st->n_seq + R >= 0x7fffffffull) { mahip_set_error("mahip_paf_stream_piece_mem: too many names"); return -1; }
	// growth is decided here, before the fold: the table is at most half full after it whatever the piece brings
	if (st->cap == 0 || 2 * ((uint64_t)st->n_seq + R) > st->cap) {
		uint32_t cap = st->cap;
		if (cap == 0) {
			cap = 1u << 16;
			if (const char *e = getenv("MA_STREAM_DICT_CAP_LOG2")) { const int l2 = atoi(e); if (l2 >= 4 && l2 <= 31) cap = 1u << l2; }
			if (2 * ((uint64_t)st->n_seq + R) > cap) cap = pow2_at_least(4 * ((uint64_t)st->n_seq + R));
		} else {
			const uint32_t want = pow2_at_least(4 * ((uint64_t)st->n_seq + R));
			cap = cap < 0x20000000u ? cap << 2 : 0x80000000u;
			if (want > cap) cap = want;
		}
		CHK(stream_table(c, st, cap));
	}
	// per local name: l2g | slot_of | blen | bpos (is_new and its scan live in the context's keep / pos)
	CHK(dev_reserve(c, st->fold, ((size_t)R + 16) * 16));
	CHK(dev_reserve(c, c->keep, ((size_t)R + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)R + 16) * 4));
	uint32_t *l2g = P<uint32_t>(st->fold), *slot_of = l2g + R, *blen = slot_of + R, *bpos = blen + R;
	uint32_t *is_new = P<uint32_t>(c->keep), *pos = P<uint32_t>(c->pos);
	const unsigned char *lnames = (const unsigned char*)b->names.p;
	const uint32_t *lpos = (const uint32_t*)b->name_pos.p, *llen = (const uint32_t*)b->name_len.p, *lseq = (const uint32_t*)b->seq_len.p;
	for (int repeat = 0;; ++repeat) {
		if (repeat > 16) { mahip_set_error("mahip_paf_stream_piece_mem: the fold ran out of probes on %d tables", repeat); return -1; } // (every repeat has 4 x the slots: 14 lead from 16 to 2^31)
		CHK(ctr_zero(c));
		hipLaunchKernelGGL(k_stream_fold, dim3(grid_for(R, 256, 8192)), dim3(256), 0, c->st, lnames, lpos, llen, R, P<unsigned long long>(st->tab), st->cap - 1, (const unsigned char*)P<unsigned char>(st->arena),
		                   (const uint32_t*)P<uint32_t>(st->name_pos), (const uint32_t*)P<uint32_t>(st->name_len), l2g, slot_of, is_new, blen, P<unsigned long long>(c->ctr));
		CHK(ctr_fetch(c));
		if (c->h_ctr[PC_OVERFLOW] == 0) break;
		if (st->cap >= 0x80000000u) { mahip_set_error("mahip_paf_stream_piece_mem: name table overflow"); return -1; }
		++sr.n_fold_repeats; // the claims of this launch die with the old table
		CHK(stream_table(c, st, st->cap < 0x20000000u ? st->cap << 2 : 0x80000000u));
	}
	uint32_t tot[2] = { 0, 0 }; // new names, their bytes in the arena
	CHK(scan_exclusive_u32(c, is_new, pos, R, P<uint32_t>(b->scal)));
	CHK(scan_exclusive_u32(c, blen, bpos, R, P<uint32_t>(b->scal) + 1));
	CHK(fetch_bytes(c, b->scal.p, tot, 8));
	if ((uint64_t)st->arena_bytes + tot[1] >= 0xffffffffull) { mahip_set_error("mahip_paf_stream_piece_mem: more than 2^32 bytes of names"); return -1; }
	const size_t ids = (size_t)st->n_seq, ids_new = ids + tot[0];
	int grew_arena = 0, grew_ids = 0;
	CHK(stream_grow(c, st->arena, st->arena_bytes, st->arena_bytes + tot[1] + 16, &grew_arena));
	CHK(stream_grow(c, st->seq_len, ids * 4, (ids_new + 4) * 4, &grew_ids)); CHK(stream_grow(c, st->name_pos, ids * 4, (ids_new + 4) * 4, &grew_ids)); CHK(stream_grow(c, st->name_len, ids * 4, (ids_new + 4) * 4, &grew_ids));
	sr.n_arena_grow += grew_arena; sr.n_ids_grow += grew_ids;
	if (st->no_cont) { // the flags grow with the per-id arrays: the flags so far are copied, the bytes behind them start as 0
		const void *was = st->excl.p;
		int grew_flags = 0;
		CHK(stream_grow(c, st->excl, ids, ids_new + 16, &grew_flags));
		if (st->excl.p != was) HIPCHK(hipMemsetAsync((char*)st->excl.p + ids, 0, st->excl.cap - ids, c->st));
		st->xrep.n_flag_grow += grew_flags;
	}
	hipLaunchKernelGGL(k_stream_commit, dim3(grid_for(R, 256)), dim3(256), 0, c->st, lnames, lpos, llen, lseq, R, (const uint32_t*)is_new, (const uint32_t*)pos, (const uint32_t*)bpos, (const uint32_t*)slot_of,
	                   st->n_seq, (uint32_t)st->arena_bytes, P<unsigned long long>(st->tab), P<unsigned char>(st->arena), P<uint32_t>(st->name_pos), P<uint32_t>(st->name_len), P<uint32_t>(st->seq_len), l2g);
	CHK(dev_reserve(c, st->map, (size_t)ps.cap_used * 4 + 16));
	hipLaunchKernelGGL(k_stream_map, dim3(grid_for(ps.cap_used, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(b->tmin), (const uint32_t*)P<uint32_t>(b->slot_id), ps.cap_used, (const uint32_t*)l2g,
	                   P<uint32_t>(st->map));
	st->n_seq += tot[0]; st->arena_bytes += tot[1];
	sr.last_local = R; sr.last_new = tot[0];
	ps.slot_to_id = (const uint32_t*)P<uint32_t>(st->map);
	return 0;
}

static double stream_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static PafStream *stream_of(mahip_ctx *c, const char *who, bool must_be_active)
{
	PafBufs *b = (PafBufs*)c->paf;
	PafStream *st = b ? b->stream : nullptr;
	if (!st || (must_be_active && !st->active)) { mahip_set_error("%s: no stream in this context (mahip_paf_stream_begin first)", who); return nullptr; }
	return st;
}

extern "C" int mahip_paf_stream_begin(mahip_ctx_t *c, int min_span, int min_match, int bi_dir)
{
	return mahip_paf_stream_begin_excl(c, min_span, min_match, bi_dir, 0, 0, 0.f);
}

extern "C" int mahip_paf_stream_begin_excl(mahip_ctx_t *c, int min_span, int min_match, int bi_dir, int no_cont, int max_hang, float int_frac)
{
	HIPCHK(hipSetDevice(c->dev));
	if (mahip_comm_active(c)) { mahip_set_error("mahip_paf_stream_begin: a context with a communicator parses ranges (mahip_paf_parse_sharded), not a stream"); return -1; }
	PafBufs *b = paf_of(c);
	HIPCHK(hipStreamSynchronize(c->st));
	paf_stream_free(c, b);
	PafStream *st = b->stream = new PafStream();
	st->active = true; st->min_span = min_span; st->min_match = min_match; st->bi_dir = bi_dir != 0;
	if (no_cont) {
		st->no_cont = 1; st->max_hang = max_hang; st->int_frac = int_frac;
		if (const char *e = getenv("MA_STREAM_NOCONT_EARLY")) st->early = atoi(e) != 0; // tests: 0 = every line waits for the end of the stream (the same result)
	}
	b->n_seq = 0; b->name_bytes = 0; b->loaded = false;
	b->parsed = false; b->rep = {}; b->odd_snap.clear();
	return 0;
}

extern "C" int mahip_paf_stream_piece_mem(mahip_ctx_t *c, const void *text, size_t nbytes, int last)
{
	HIPCHK(hipSetDevice(c->dev));
	PafStream *st = stream_of(c, "mahip_paf_stream_piece_mem", true);
	if (!st) return -1;
	PafBufs *b = paf_of(c);
	mahip_paf_stream_report_t &sr = st->rep;
	if (st->closed) { mahip_set_error("mahip_paf_stream_piece_mem: a piece behind the last piece"); return -1; }
	if (nbytes && !last && ((const char*)text)[nbytes - 1] != '\n') { mahip_set_error("mahip_paf_stream_piece_mem: a piece that is not the last must end with a newline (pieces are whole lines)"); return -1; }
	++sr.n_pieces;
	if (last) st->closed = true;
	if (!nbytes) { ++sr.n_empty; return 0; }
	const double t0 = stream_now();
	// ---- the piece's text (MA_PAF_MAX_BYTES counts its own bytes)
	CHK(paf_reserve_text(c, nbytes));
	CHK(xfer_copy(c, b->text.p, (void*)text, nbytes, 1));
	b->loaded = true;
	const double t1 = stream_now();
	// ---- the stages of a whole parse on the piece
	b->parsed = false; b->rep = {}; b->odd_snap.clear();
	mahip_paf_report_t &rp = b->rep;
	PafParse ps;
	CHK(paf_census(c, b, ps));
	if (st->n_lines + ps.L + 1 >= 0x7fffffffull) { mahip_set_error("mahip_paf_parse: more than 2^31 lines"); return -1; }
	CHK(paf_reserve_cols(c, b, ps));
	CHK(paf_fields(c, b, ps, st->min_span, st->min_match));
	rp.n_lines = ps.L; rp.n_gran = ps.n_gran; rp.tile_k = ps.tile_k; rp.n_tiles = ps.n_tiles; rp.open_line = ps.open_line; rp.n_long = ps.n_long;
	// ---- the stale bl (paf.c:54): a 10-column line in front of the piece's first 11-column line inherits from the last such line of ANY earlier piece (0 before the first)
	const uint32_t before = st->have_bl ? st->last_bl : 0u;
	sr.last_before = before;
	if (ps.L && ps.n_valid) {
		uint32_t lb[3] = { 0, 0, 0 };
		hipLaunchKernelGGL(k_stream_last_bl, dim3(1), dim3(64), 0, c->st, (const uint8_t*)ps.o.flags, (const uint32_t*)ps.o.bl, ps.L, P<uint32_t>(b->scal) + 4);
		CHK(fetch_bytes(c, P<uint32_t>(b->scal) + 4, lb, 12));
		if (ps.n_nobl) {
			rp.bl_pass = 1;
			CHK(paf_stale_bl(c, b, ps, false, before));
			if (st->have_bl && (lb[2] & 5u) == 1u) ++sr.n_inherited; // its first line is a 10-column line, and an earlier piece had left a bl
		}
		if (lb[0]) { st->have_bl = true; st->last_bl = lb[1]; }
	}
	double t_fold = 0.0;
	// ---- names and records
	sr.last_local = sr.last_new = 0;
	if (ps.n_pass) {
		CHK(paf_dict_local(c, b, ps, 0, 0, 0.f));
		const double f0 = stream_now();
		CHK(paf_stream_fold(c, b, st, ps));
		t_fold = stream_now() - f0;
		uint32_t *cnt = nullptr, *cpos = nullptr;
		if (st->no_cont) { // hit.c:38-68 on the piece's stored lines, then the lines that touch a flagged name go (k_stream_verdict)
			const uint32_t L = ps.L;
			CHK(dev_reserve(c, c->keep, ((size_t)L + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)L + 16) * 4));
			cnt = P<uint32_t>(c->keep); cpos = P<uint32_t>(c->pos);
			hipLaunchKernelGGL(k_stream_verdict, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, ps.o, L, ps.slot_to_id, st->max_hang, st->int_frac, P<uint8_t>(st->excl));
			CHK(ctr_zero(c));
			hipLaunchKernelGGL(k_stream_early, dim3(grid_for(L, 256, 8192)), dim3(256), 0, c->st, ps.o, L, ps.slot_to_id, (const uint8_t*)P<uint8_t>(st->excl), st->early, st->bi_dir, cnt,
			                   P<unsigned long long>(c->ctr));
			CHK(ctr_fetch(c));
			st->xrep.n_early_lines += ps.n_pass - (size_t)c->h_ctr[PC_PASS];
			ps.n_pass = (size_t)c->h_ctr[PC_PASS];
		}
		const size_t max_hits = st->bi_dir ? 2 * ps.n_pass : ps.n_pass;
		if (st->n_rec + max_hits >= 0xffffffffull) { mahip_set_error("mahip_paf_parse: more than 2^32 records"); return -1; }
		if (st->rec_cap == 0) { // the first capacity
			st->rec_cap = (size_t)1 << 20;
			if (const char *e = getenv("MA_STREAM_REC_CAP")) { const long long v = atoll(e); if (v >= 1) st->rec_cap = (size_t)v; }
			CHK(dev_reserve(c, st->rec, (st->rec_cap + 1) * sizeof(ma_hit_t)));
			if (st->no_cont) CHK(dev_reserve(c, st->lens, (st->rec_cap + 1) * sizeof(uint2)));
		}
		if (st->n_rec + max_hits > st->rec_cap) {
			size_t want = 2 * st->rec_cap;
			if (want < st->n_rec + max_hits) want = st->n_rec + max_hits;
			CHK(stream_grow(c, st->rec, st->n_rec * sizeof(ma_hit_t), (want + 1) * sizeof(ma_hit_t)));
			if (st->no_cont) { // the lengths column grows with the record buffer
				int grew_lens = 0;
				CHK(stream_grow(c, st->lens, st->n_rec * sizeof(uint2), (want + 1) * sizeof(uint2), &grew_lens));
				st->xrep.n_lens_grow += grew_lens;
			}
			st->rec_cap = want;
			++sr.n_rec_grow;
		}
		if (st->no_cont && ps.n_pass) { // (the piece's records take [n_rec, n_rec + the scanned total), and that total is at most max_hits)
			CHK(scan_exclusive_u32(c, cnt, cpos, ps.L, P<uint32_t>(b->scal) + 1));
			hipLaunchKernelGGL(k_stream_lens, dim3(grid_for(ps.L, 256, 8192)), dim3(256), 0, c->st, ps.o, ps.L, (const uint32_t*)cnt, (const uint32_t*)cpos, (uint2*)st->lens.p + st->n_rec);
		}
		if (ps.n_pass) CHK(paf_records(c, b, ps, st->bi_dir, (ma_hit_t*)st->rec.p + st->n_rec));
		st->n_rec += ps.n_hits;
		if (st->n_rec > st->xrep.peak_records) st->xrep.peak_records = st->n_rec;
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->st));
	// ---- the running totals
	st->n_lines += ps.L; st->n_valid += ps.n_valid; st->n_pass += ps.n_pass;
	if (ps.max_qs > st->max_qs) st->max_qs = ps.max_qs;
	st->any_parsed = true;
	sr.last_form = rp.dict_form;
	sr.n_short += rp.dict_form == MAHIP_PAF_DICT_SHORT; sr.n_text += rp.dict_form == MAHIP_PAF_DICT_TEXT;
	sr.tab_cap = st->cap;
	const double t3 = stream_now();
	sr.t_upload += t1 - t0; sr.t_fold += t_fold; sr.t_parse += (t3 - t1) - t_fold;
	return 0;
}

// -R at the end of the stream: what the flags of all pieces leave of the records and of the dictionary, renumbered by first appearance among the surviving
// lines (hit.c:86-90: the second pass hands out ids only for lines that pass).  Replaces st->rec, st->arena and the per-id arrays; sets the totals.
static int paf_stream_retire(mahip_ctx *c, PafBufs *b, PafStream *st, uint32_t *n_excl)
{
	mahip_paf_stream_excl_report_t &xr = st->xrep;
	unsigned long long *ctr = P<unsigned long long>(c->ctr);
	const size_t n_rec = st->n_rec;
	const uint32_t n_seq = st->n_seq;
	*n_excl = 0;
	if (n_seq == 0) return 0; // no line was ever stored: no name, no flag, no record
	const uint8_t *excl = (const uint8_t*)P<uint8_t>(st->excl);
	CHK(ctr_zero(c));
	hipLaunchKernelGGL(k_excl_count, dim3(grid_for(n_seq, 256, 2048)), dim3(256), 0, c->st, excl, n_seq, ctr);
	CHK(ctr_fetch(c));
	xr.n_flagged = *n_excl = (uint32_t)c->h_ctr[PC_VALID];
	// ---- dead records; the first surviving appearance of every id
	ScopedDev first(c), alive(c), new_id(c);
	CHK(dev_reserve(c, first.b, ((size_t)n_seq + 2) * 8)); CHK(dev_reserve(c, alive.b, (n_rec + 16) * 4)); CHK(dev_reserve(c, new_id.b, ((size_t)n_seq + 4) * 4));
	HIPCHK(hipMemsetAsync(first.b.p, 0xff, (size_t)n_seq * 8, c->st));
	CHK(ctr_zero(c));
	if (n_rec) hipLaunchKernelGGL(k_stream_mark, dim3(grid_for(n_rec, 256, 8192)), dim3(256), 0, c->st, (const uint4*)st->rec.p, n_rec, excl, (unsigned long long*)first.b.p, (uint32_t*)alive.b.p, ctr);
	CHK(ctr_fetch(c));
	const size_t n_alive = (size_t)c->h_ctr[PC_PASS], n_self = (size_t)c->h_ctr[PC_VALID];
	const size_t lines_alive = st->bi_dir ? (n_alive - n_self) / 2 + n_self : n_alive; // hit.c:87-98: two records a line, one for a self hit
	xr.n_late_records = n_rec - n_alive; xr.n_late_lines = st->n_pass - lines_alive;
	// ---- the survivors' new ids: the ranks of their first appearances
	uint32_t R = 0, nb = 0, n_keep = 0;
	CHK(dev_reserve(c, c->keep, ((size_t)n_seq + 16) * 4)); CHK(dev_reserve(c, c->pos, ((size_t)n_seq + 16) * 4));
	hipLaunchKernelGGL(k_stream_id_flag, dim3(grid_for(n_seq, 256)), dim3(256), 0, c->st, (const unsigned long long*)first.b.p, n_seq, P<uint32_t>(c->keep));
	CHK(scan_exclusive_u32(c, P<uint32_t>(c->keep), P<uint32_t>(c->pos), n_seq, P<uint32_t>(b->scal)));
	CHK(fetch_u32(c, b->scal.p, &R));
	for (int k = 0; k < 2; ++k) { CHK(dev_reserve(c, c->key[k], ((size_t)R + 1) * 8)); CHK(dev_reserve(c, c->val[k], ((size_t)R + 1) * 4)); }
	hipLaunchKernelGGL(k_stream_id_collect, dim3(grid_for(n_seq, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(c->keep), (const uint32_t*)P<uint32_t>(c->pos), (const unsigned long long*)first.b.p, n_seq,
	                   P<uint64_t>(c->key[0]), P<uint32_t>(c->val[0]));
	int gen = 0;
	if (R) CHK(radix_sort_pairs(c, R, 0, bitlen_u64(2ull * n_rec), 0, 0, &gen));
	// ---- the dictionary in new-id order: R <= n_seq names, their bytes (<= arena_bytes) out of the old arena
	DevBuf arena2, pos2, len2, seq2, rec2;
	auto give_up = [&]() { (void)hipStreamSynchronize(c->st); dev_free(c, arena2); dev_free(c, pos2); dev_free(c, len2); dev_free(c, seq2); dev_free(c, rec2); return -1; };
#define CHK2(x) do { if ((x) != 0) return give_up(); } while (0)
	CHK2(dev_reserve(c, pos2, ((size_t)R + 4) * 4)); CHK2(dev_reserve(c, len2, ((size_t)R + 4) * 4)); CHK2(dev_reserve(c, seq2, ((size_t)R + 4) * 4));
	CHK2(dev_reserve(c, c->keep, ((size_t)R + 16) * 4));
	if (R) hipLaunchKernelGGL(k_stream_id_assign, dim3(grid_for(R, 256)), dim3(256), 0, c->st, (const uint64_t*)P<uint64_t>(c->key[gen]), (const uint32_t*)P<uint32_t>(c->val[gen]), R,
	                          (const uint32_t*)P<uint32_t>(st->name_len), (const uint2*)st->lens.p, (uint32_t*)new_id.b.p, (uint32_t*)len2.p, (uint32_t*)seq2.p, P<uint32_t>(c->keep));
	CHK2(scan_exclusive_u32(c, P<uint32_t>(c->keep), (uint32_t*)pos2.p, R, P<uint32_t>(b->scal)));
	CHK2(fetch_u32(c, b->scal.p, &nb));
	CHK2(dev_reserve(c, arena2, (size_t)nb + 16));
	if (R) hipLaunchKernelGGL(k_stream_names, dim3(grid_for(R, 256)), dim3(256), 0, c->st, (const unsigned char*)P<unsigned char>(st->arena), (const uint32_t*)P<uint32_t>(st->name_pos),
	                          (const uint32_t*)P<uint32_t>(c->val[gen]), (const uint32_t*)pos2.p, (const uint32_t*)len2.p, R, (unsigned char*)arena2.p);
	// ---- the surviving records, relabelled, into a second buffer (the lengths column has done its work: it goes first)
	if (hipStreamSynchronize(c->st) != hipSuccess) return give_up();
	dev_free(c, st->lens);
	CHK2(scan_exclusive_u32(c, (const uint32_t*)alive.b.p, (uint32_t*)alive.b.p, n_rec, P<uint32_t>(b->scal)));
	CHK2(fetch_u32(c, b->scal.p, &n_keep));
	if (n_keep != n_alive) { mahip_set_error("mahip_paf_stream_end: %u records survive the scan, %zu the count", n_keep, n_alive); return give_up(); }
	CHK2(dev_reserve(c, rec2, ((size_t)n_keep + 1) * sizeof(ma_hit_t)));
	if (n_rec) hipLaunchKernelGGL(k_stream_compact, dim3(grid_for(n_rec, 256, 8192)), dim3(256), 0, c->st, (const uint4*)st->rec.p, n_rec, excl, (const uint32_t*)alive.b.p, (const uint32_t*)new_id.b.p, (uint4*)rec2.p);
	{ hipError_t le = hipGetLastError(); if (le != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) { mahip_set_error("mahip_paf_stream_end: %s", hipGetErrorString(le)); return give_up(); } }
#undef CHK2
	dev_free(c, st->rec); dev_free(c, st->arena); dev_free(c, st->name_pos); dev_free(c, st->name_len); dev_free(c, st->seq_len);
	st->rec = rec2; st->arena = arena2; st->name_pos = pos2; st->name_len = len2; st->seq_len = seq2;
	st->n_rec = n_keep; st->n_seq = R; st->arena_bytes = nb; st->n_pass = lines_alive;
	xr.n_renumbered = R;
	return 0;
}

extern "C" int mahip_paf_stream_end(mahip_ctx_t *c, mahip_paf_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	PafStream *st = stream_of(c, "mahip_paf_stream_end", true);
	if (!st) return -1;
	PafBufs *b = paf_of(c);
	memset(info, 0, sizeof(*info));
	HIPCHK(hipStreamSynchronize(c->st));
	uint32_t n_excl = 0;
	if (st->no_cont) CHK(paf_stream_retire(c, b, st, &n_excl));
	// the dictionary and the records change hands: they are laid out as a whole parse leaves them
	dev_free(c, b->names); dev_free(c, b->name_pos); dev_free(c, b->seq_len); dev_free(c, b->name_len); dev_free(c, c->aos_own);
	b->names = st->arena; b->name_pos = st->name_pos; b->seq_len = st->seq_len; b->name_len = st->name_len; c->aos_own = st->rec;
	st->arena = DevBuf(); st->name_pos = DevBuf(); st->seq_len = DevBuf(); st->name_len = DevBuf(); st->rec = DevBuf();
	dev_free(c, st->tab); dev_free(c, st->fold); dev_free(c, st->map); dev_free(c, st->excl); dev_free(c, st->lens);
	b->n_seq = st->n_seq; b->name_bytes = st->arena_bytes;
	PafParse ps;
	ps.n_hits = st->n_rec; ps.R = st->n_seq;
	CHK(paf_adopt(c, ps));
	HIPCHK(hipStreamSynchronize(c->st));
	c->hint_max_qs = c->paf_max_qs = st->max_qs;
	c->run_stride = st->bi_dir ? 2 : 1; // still a line's record and its mirror side by side, in line order
	b->parsed = true; // (mahip_paf_last / mahip_paf_cols_download: the last piece that had text; zeros when none had)
	b->loaded = false;
	info->n_records = st->n_valid; info->n_stored_lines = st->n_pass; info->n_hits = st->n_rec; info->n_seq = st->n_seq; info->max_qs = st->max_qs;
	info->name_bytes = st->arena_bytes; info->n_lines = st->n_lines;
	b->rep.n_excl = info->n_excl = n_excl;
	st->active = false;
	return 0;
}

extern "C" int mahip_paf_stream_abort(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	PafBufs *b = (PafBufs*)c->paf;
	if (!b || !b->stream) return 0;
	HIPCHK(hipStreamSynchronize(c->st));
	paf_stream_free(c, b);
	b->loaded = false; b->parsed = false;
	return 0;
}

extern "C" int mahip_paf_stream_last(mahip_ctx_t *c, mahip_paf_stream_report_t *out)
{
	PafStream *st = stream_of(c, "mahip_paf_stream_last", false);
	if (!st) return -1;
	if (out) *out = st->rep;
	return 0;
}

extern "C" int mahip_paf_stream_excl_last(mahip_ctx_t *c, mahip_paf_stream_excl_report_t *out)
{
	PafStream *st = stream_of(c, "mahip_paf_stream_excl_last", false);
	if (!st) return -1;
	if (out) *out = st->xrep;
	return 0;
}

extern "C" int mahip_paf_stream_tab_download(mahip_ctx_t *c, uint64_t *slots)
{
	HIPCHK(hipSetDevice(c->dev));
	PafStream *st = stream_of(c, "mahip_paf_stream_tab_download", true);
	if (!st) return -1;
	if (st->cap) CHK(fetch_bytes(c, st->tab.p, slots, (size_t)st->cap * 8));
	return 0;
}

extern "C" int mahip_paf_names(mahip_ctx_t *c, char *names, uint32_t *lens)
{
	HIPCHK(hipSetDevice(c->dev));
	PafBufs *b = paf_of(c);
	if (b->n_seq == 0) return 0;
	if (names) CHK(xfer_copy(c, b->names.p, names, b->name_bytes, 0));
	if (lens) CHK(xfer_copy(c, b->seq_len.p, lens, (size_t)b->n_seq * 4, 0));
	return 0;
}

// The host dictionary without per-name host work: sd_seq_t records (sdict.h:6-10: name pointer, len, aux:31 | del:1 -- 16 bytes) written by the
// device FOR the block the names are about to be copied into (names_host: its address on the host), so that both arrive as two plain copies.
__global__ __launch_bounds__(256) void k_dict_seqs(unsigned long long names_host, const uint32_t *__restrict__ name_pos, const uint32_t *__restrict__ seq_len, uint32_t R,
                                                    uint4 *__restrict__ out, unsigned long long *__restrict__ ctr)
{
	uint64_t tot = 0;
	for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < R; j += gridDim.x * 256u) {
		const unsigned long long p = names_host + name_pos[j];
		out[j] = make_uint4((uint32_t)p, (uint32_t)(p >> 32), seq_len[j], 0u);
		tot += seq_len[j];
	}
	blk_add_u64(&ctr[PC_VALID], tot);
}
extern "C" int mahip_paf_seqs(mahip_ctx_t *c, char *names, void *seqs16, uint64_t *tot_len)
{
	HIPCHK(hipSetDevice(c->dev));
	PafBufs *b = paf_of(c);
	if (tot_len) *tot_len = 0;
	if (b->n_seq == 0) return 0;
	const uint32_t R = b->n_seq;
	CHK(dev_reserve(c, c->key[0], ((size_t)R + 1) * 16));
	CHK(ctr_zero(c));
	hipLaunchKernelGGL(k_dict_seqs, dim3(grid_for(R, 256, 1024)), dim3(256), 0, c->st, (unsigned long long)(uintptr_t)names, (const uint32_t*)P<uint32_t>(b->name_pos),
	                   (const uint32_t*)P<uint32_t>(b->seq_len), R, (uint4*)c->key[0].p, P<unsigned long long>(c->ctr));
	CHK(ctr_fetch(c));
	if (tot_len) *tot_len = c->h_ctr[PC_VALID];
	CHK(xfer_copy(c, b->names.p, names, b->name_bytes, 0));
	CHK(xfer_copy(c, c->key[0].p, seqs16, (size_t)R * 16, 0));
	return 0;
}

// ---- for stage tests: what the last parse decided, and its per-line columns (valid from mahip_paf_parse* to mahip_paf_release)
extern "C" int mahip_paf_keep_odd(mahip_ctx_t *c, int on)
{
	c->paf_keep_odd = on != 0;
	return 0;
}
static PafBufs *paf_parsed(mahip_ctx *c, const char *who)
{
	PafBufs *b = (PafBufs*)c->paf;
	if (!b || !b->parsed) { mahip_set_error("%s: no parsed text in this context (not parsed yet, or released)", who); return nullptr; }
	return b;
}
extern "C" int mahip_paf_last(mahip_ctx_t *c, mahip_paf_report_t *out)
{
	PafBufs *b = paf_parsed(c, "mahip_paf_last");
	if (!b) return -1;
	if (out) *out = b->rep;
	return 0;
}
extern "C" int mahip_paf_cols_download(mahip_ctx_t *c, uint8_t *flags, uint8_t *odd, uint32_t *nums, uint32_t *tnoff, uint32_t *qlen, uint32_t *tlen, uint64_t *lstart, uint64_t *tfirst)
{
	HIPCHK(hipSetDevice(c->dev));
	PafBufs *b = paf_parsed(c, "mahip_paf_cols_download");
	if (!b) return -1;
	const size_t L = (size_t)b->rep.n_lines;
	if (odd) {
		if (b->odd_snap.size() != L) { mahip_set_error("mahip_paf_cols_download: no snapshot of the odd lines (mahip_paf_keep_odd was off during the parse)"); return -1; }
		if (L) memcpy(odd, b->odd_snap.data(), L);
	}
	if (L == 0) return 0;
	if (flags) CHK(xfer_copy(c, b->flags.p, flags, L, 0));
	if (nums) for (int k = 0; k < 8; ++k) CHK(xfer_copy(c, b->num[k].p, nums + (size_t)k * L, L * 4, 0));
	if (tnoff) CHK(xfer_copy(c, b->tnoff.p, tnoff, L * 4, 0));
	if (qlen) CHK(xfer_copy(c, b->qlen.p, qlen, L * 4, 0));
	if (tlen) CHK(xfer_copy(c, b->tlen.p, tlen, L * 4, 0));
	if (lstart) CHK(xfer_copy(c, b->lstart.p, lstart, (L + 1) * 8, 0));
	if (tfirst && b->rep.n_tiles) CHK(xfer_copy(c, b->tfirst.p, tfirst, (size_t)b->rep.n_tiles * 8, 0));
	return 0;
}

// the text and the per-line columns are only needed until the records and the names are out
extern "C" int mahip_paf_release(mahip_ctx_t *c)
{
	HIPCHK(hipSetDevice(c->dev));
	HIPCHK(hipStreamSynchronize(c->st));
	paf_free(c);
	return 0;
}

extern "C" uint32_t mahip_paf_max_qs(mahip_ctx_t *c) { return c->paf_max_qs; }
