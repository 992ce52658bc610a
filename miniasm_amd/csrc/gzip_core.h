/* gzip_core.h -- a plain gzip member's ONE deflate stream inflated by many waves (csrc/xfer.hip: k_gz_sync_count, k_gz_heads, k_gz_decode).
 * Concatenated members are one stream each: k_gz_heads starts a wave at the first bit behind a later member's header exactly as chunk 0's wave starts at bit 0.
 *
 * The payload is cut into chunks of C bytes.  A wave's coordinates are LOCAL: bit 0 is the first bit of its chunk, `in` points there, and in_len is cut at
 * GZ_SPAN_MAX + 2 chunks + GZ_BLOCK_MAX bytes (or the end of the payload), so one wave reads a bounded piece of the input whatever the stream holds.
 *
 *   gz_holds     ONE LANE: do the bits at `bit` begin a dynamic block's header that holds (the rules of inf_dynamic / inf_tables, decided from the Kraft sums
 *                alone: no tables are built)?  Reads the input itself, bytewise, below in_len only; every loop in it is counted (19 lengths, HLIT + HDIST <=
 *                316 lengths, each step advancing by >= 1).
 *   gz_item      THE WAVE: decodes block after block from a block start with inflate_core.h's bit reader and tables.  WRITE = false sums the output length and
 *                writes nothing; WRITE = true writes 16-bit symbols (a literal, or GZ_REF | cell of the 32 KiB window in front of the item) through a ring of
 *                the last 32768 symbols in LDS, flushed 8 KiB at a time exactly as inflate_core.h flushes its bytes.
 *
 * TERMINATION: as inflate_core.h -- every block consumes >= 3 bits, every symbol >= 1, a code longer than what is left is INF_IN_EXHAUSTED, and the input a wave
 * may read is bounded as said above.  BOUNDS: input below in_len, symbols below o.lim (the item's counted length), both checked before the access; the ring is
 * indexed modulo its size.  Lanes share LDS across wv_sync() only, as there. */
#ifndef MA_GZIP_CORE_H
#define MA_GZIP_CORE_H
#include "inflate_core.h"

#define GZ_SPAN_MAX 16u          /* an item may run over this many whole chunks without a block start of its own chunk's successor */
#define GZ_BLOCK_MAX (1u << 20)  /* input bytes behind the span that a wave may still read: the longest block that may straddle the end of a span */
#define GZ_WIN 32768u
#define GZ_REF 0x8000u
#define GZ_NO_SYNC (INF_CRC + 1) /* a kernel status of its own */
#define GZ_UNCONFIRMED 0xffu     /* gz_item: the candidate's first block did not hold up (never stored in a row) */

struct GzLds : InfTabs { uint16_t ring[GZ_WIN]; };                /* k_gz_decode: 69 KiB a wave, two waves to a CU */
struct GzCand { uint8_t cnt[64][8]; uint8_t sym[64][24]; };       /* k_gz_sync_count: every lane's code-length code */
struct GzOut { uint64_t op, fp, lim, before; uint16_t *out; };    /* symbols produced / flushed / the most there may be; text bytes in front of the item */

/* up to 24 bits at `bit`, zero-filled behind the input */
__device__ __forceinline__ uint32_t gz_peek(const uint8_t *in, uint32_t in_len, uint64_t bit, uint32_t n)
{
	const uint64_t by = bit >> 3;
	uint32_t w = 0;
	for (uint32_t k = 0; k < 4; ++k) if (by + k < in_len) w |= (uint32_t)in[by + k] << (8 * k);
	return (w >> (bit & 7u)) & ((1u << n) - 1u);
}

__device__ __forceinline__ bool gz_holds(const uint8_t *in, uint32_t in_len, uint64_t bit, uint8_t *ccnt, uint8_t *csym)
{
	const uint64_t nbits = (uint64_t)in_len * 8;
	if (bit + 17 > nbits) return false;
	const uint32_t h = gz_peek(in, in_len, bit, 17);
	if (((h >> 1) & 3u) != 2u) return false;
	const uint32_t hlit = ((h >> 3) & 31u) + 257, hdist = ((h >> 8) & 31u) + 1, hclen = (h >> 13) + 4;
	if (hlit > 286 || hdist > 30) return false;
	bit += 17;
	if (bit + 3 * hclen > nbits) return false;
	uint64_t cl = 0; /* the 19 lengths of the code-length code, three bits each, by symbol */
	for (uint32_t k = 0; k < hclen; ++k) {
		const uint32_t o = (uint32_t)((k < 12 ? INF_ORD_A >> (5 * k) : INF_ORD_B >> (5 * (k - 12))) & 31u);
		cl |= (uint64_t)gz_peek(in, in_len, bit, 3) << (3 * o);
		bit += 3;
	}
	for (uint32_t l = 0; l < 8; ++l) ccnt[l] = 0;
	for (uint32_t s = 0; s < 19; ++s) ++ccnt[(cl >> (3 * s)) & 7u];
	int left = 1;
	for (uint32_t l = 1; l < 8; ++l) { left = 2 * left - (int)ccnt[l]; if (left < 0) return false; }
	if (left != 0) return false; /* inf_dynamic takes a complete code-length code only */
	uint32_t idx = 0;
	for (uint32_t l = 1; l < 8; ++l) for (uint32_t s = 0; s < 19; ++s) if (((cl >> (3 * s)) & 7u) == l) csym[idx++] = (uint8_t)s;
	/* the HLIT + HDIST lengths: only their Kraft sums (in units of 2^-15), the longest of each and symbol 256 are kept */
	const uint32_t total = hlit + hdist;
	uint32_t lsum = 0, dsum = 0, lmax = 0, dmax = 0, prev = 0, has256 = 0;
	for (uint32_t i = 0; i < total;) {
		uint32_t b = gz_peek(in, in_len, bit, 7), code = 0, first = 0, index = 0, sym = 99, len;
		for (len = 1; len < 8; ++len) {
			code |= b & 1u; b >>= 1;
			const uint32_t cnt = ccnt[len];
			if (code < first + cnt) { sym = csym[index + (code - first)]; break; }
			index += cnt; first += cnt; first <<= 1; code <<= 1;
		}
		if (sym == 99) return false;
		bit += len;
		uint32_t rep = 1, val = sym;
		if (sym == 16) { if (i == 0) return false; rep = 3 + gz_peek(in, in_len, bit, 2); bit += 2; val = prev; }
		else if (sym == 17) { rep = 3 + gz_peek(in, in_len, bit, 3); bit += 3; val = 0; }
		else if (sym == 18) { rep = 11 + gz_peek(in, in_len, bit, 7); bit += 7; val = 0; }
		if (bit > nbits || rep > total - i) return false;
		const uint32_t e = i + rep, nl = (e < hlit ? e : hlit) - (i < hlit ? i : hlit), nd = rep - nl;
		if (val) {
			lsum += nl << (15 - val); dsum += nd << (15 - val);
			if (nl && val > lmax) lmax = val;
			if (nd && val > dmax) dmax = val;
		}
		if (i <= 256 && 256 < e) has256 = val != 0;
		i = e; prev = val;
	}
	if (!has256) return false;
	if (lsum > 32768u || (lsum < 32768u && lmax != 1)) return false; /* inf_tables: over-subscribed never, incomplete only as one code of one bit */
	if (dsum > 32768u || (dsum < 32768u && dmax > 1)) return false;
	return true;
}

/* the bit reader at local bit `bit` */
__device__ __forceinline__ void gz_seek(InfState &s, InfTabs &L, uint64_t bit)
{
	s.ip = s.lp = (uint32_t)(bit >> 3); s.bitbuf = 0; s.bitcnt = 0; s.err = INF_OK; s.fixed = 0;
	if (bit & 7u) (void)inf_bits(s, L, (uint32_t)(bit & 7u));
}
__device__ __forceinline__ uint64_t gz_pos(const InfState &s) { return (uint64_t)s.ip * 8 - s.bitcnt; }

__device__ __forceinline__ void gz_flush(InfState &s, uint16_t *ring, GzOut &o)
{
	wv_sync();
	for (uint64_t p = o.fp + s.lane; p < o.op; p += 64) o.out[p] = ring[p & (GZ_WIN - 1)];
	o.fp = o.op;
}

template <bool WRITE> __device__ __forceinline__ void gz_stored(InfState &s, InfTabs &L, uint16_t *ring, GzOut &o)
{
	const uint32_t drop = s.bitcnt & 7u;
	s.bitbuf >>= drop; s.bitcnt -= drop;
	const uint32_t len = inf_bits(s, L, 16), nlen = inf_bits(s, L, 16);
	if (s.err) return;
	if (len != (~nlen & 0xffffu)) { s.err = INF_STORED_LEN; return; }
	s.ip -= s.bitcnt >> 3; s.bitbuf = 0; s.bitcnt = 0;
	if (len > s.in_len - s.ip) { s.err = INF_IN_EXHAUSTED; return; }
	if (WRITE) {
		if (len > o.lim - o.op) { s.err = INF_OUT_OVERFLOW; return; }
		for (uint32_t done = 0; done < len; done += 256) {
			const uint32_t n = len - done < 256 ? len - done : 256;
			for (uint32_t k = s.lane; k < n; k += 64) ring[(o.op + k) & (GZ_WIN - 1)] = s.in[s.ip + done + k];
			o.op += n;
			if (o.op - o.fp >= INF_SEG) gz_flush(s, ring, o);
		}
	} else o.op += len;
	s.ip += len;
	if (s.lp < s.ip) s.lp = s.ip;
}

template <bool WRITE> __device__ __forceinline__ void gz_codes(InfState &s, InfTabs &L, uint16_t *ring, GzOut &o)
{
	for (;;) {
		uint32_t sym = inf_sym(s, L, L.lfast, INF_LBITS, L.lcount, L.lsym);
		if (s.err) return;
		if (sym < 256) {
			if (WRITE) {
				if (o.op >= o.lim) { s.err = INF_OUT_OVERFLOW; return; }
				if (s.lane == 0) ring[o.op & (GZ_WIN - 1)] = (uint16_t)sym;
			}
			++o.op;
		} else if (sym == 256) return;
		else {
			if (sym > 285) { s.err = INF_BAD_SYMBOL; return; }
			uint32_t len;
			if (sym < 265) len = sym - 254;
			else if (sym == 285) len = 258;
			else { const uint32_t e = (sym - 261) >> 2; len = ((4 + ((sym - 265) & 3u)) << e) + 3 + inf_bits(s, L, e); }
			const uint32_t ds = inf_sym(s, L, L.dfast, INF_DBITS, L.dcount, L.dsym);
			if (s.err) return;
			if (ds > 29) { s.err = INF_BAD_SYMBOL; return; }
			uint32_t dist;
			if (ds < 4) dist = ds + 1;
			else { const uint32_t e = (ds >> 1) - 1; dist = ((2 + (ds & 1u)) << e) + 1 + inf_bits(s, L, e); }
			if (s.err) return;
			if (WRITE) {
				/* dist <= 32768.  A source in front of the item's own output is a cell of the window in front of the item: cell 32768 - r is r bytes in
				 * front of it.  The text in front of the item is o.before bytes long: a reach beyond it is in front of the stream. */
				if (dist > o.op && dist - o.op > o.before) { s.err = INF_DIST_TOO_FAR; return; }
				if (len > o.lim - o.op) { s.err = INF_OUT_OVERFLOW; return; }
				wv_sync();
				for (uint32_t r = 0; r < len; r += 64) {
					const uint32_t k = r + s.lane;
					uint16_t v = 0;
					if (k < len) {
						const uint64_t src = o.op + (k < dist ? k : k % dist); /* + dist: the source position, kept unsigned */
						v = src >= dist ? ring[(src - dist) & (GZ_WIN - 1)] : (uint16_t)(GZ_REF | (uint32_t)(GZ_WIN - (dist - src)));
					}
					wv_sync();
					if (k < len) ring[(o.op + k) & (GZ_WIN - 1)] = v;
				}
			}
			o.op += len;
		}
		if (WRITE && o.op - o.fp >= INF_SEG) gz_flush(s, ring, o);
	}
}

/* Block after block from local bit `start`.
 * WRITE = false (k_gz_sync_count): stops at the first block start that follows a BFINAL block (*saw_final), that lies in a chunk more than GZ_SPAN_MAX whole
 *   chunks behind the item's own (GZ_NO_SYNC), or that begins a dynamic block at a bit >= chunk_bits (the next chunk's first); confirm: the first block is a
 *   candidate -- a status in it, or BTYPE 3 in the three bits behind it, returns GZ_UNCONFIRMED.
 * WRITE = true (k_gz_decode): stops at the block start at or behind `stop` (the end the count pass found).
 * Returns the status; *end = the local bit it stopped at; o.op = the output length. */
template <bool WRITE> __device__ __forceinline__ uint32_t gz_item(InfState &s, InfTabs &L, uint16_t *ring, GzOut &o, uint64_t start, uint64_t chunk_bits, uint64_t stop, bool confirm,
                                                                  uint64_t *end, uint32_t *saw_final, uint32_t nblk[3])
{
	gz_seek(s, L, start);
	uint32_t last = 0, status = INF_OK;
	bool first = true;
	*saw_final = 0;
	for (;;) {
		const uint64_t pos = gz_pos(s);
		*end = pos;
		if (s.err) { status = s.err; break; } /* (the seek itself ran out of input) */
		if (!first) {
			if (last) { *saw_final = 1; break; }
			if (WRITE) { if (pos >= stop) break; }
			else if (pos / chunk_bits > GZ_SPAN_MAX + 1) { status = GZ_NO_SYNC; break; }
		}
		last = inf_bits(s, L, 1);
		const uint32_t type = inf_bits(s, L, 2);
		if (s.err) { status = s.err; break; }
		if (!WRITE && !first && type == 2 && pos >= chunk_bits) break;
		if (type == 3) { status = INF_BAD_BTYPE; break; }
		nblk[type] += 1;
		wv_sync(); /* nobody decodes with the tables of the block before any more */
		if (type == 0) gz_stored<WRITE>(s, L, ring, o);
		else {
			if (type == 1) inf_fixed(s, L); else inf_dynamic(s, L);
			if (!s.err) gz_codes<WRITE>(s, L, ring, o);
		}
		if (s.err) { status = s.err; *end = gz_pos(s); break; }
		if (first && confirm && !last) {
			inf_refill(s, L);
			if (s.bitcnt >= 3 && (((uint32_t)s.bitbuf >> 1) & 3u) == 3u) return GZ_UNCONFIRMED;
		}
		first = false;
	}
	if (first && confirm && status != INF_OK) return GZ_UNCONFIRMED;
	return status;
}
#endif
