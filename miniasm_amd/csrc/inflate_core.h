/* inflate_core.h -- RFC 1951 inflate of ONE deflate stream (a BGZF member's payload, <= 64 KiB of output) by ONE wave; used by k_bgzf_inflate (csrc/xfer.hip).
 *
 * Symbol decoding is serial, so everything that steers it -- the bit buffer, the input and output positions, the status -- is WAVE-UNIFORM: every lane holds
 * the same values and takes the same branches.  The 64 lanes share the work that is parallel: fetching the input window, filling the decode tables, copying
 * stored bytes and matches, flushing the output.  Per wave in LDS (InfLds, 37 KiB, four waves to a 160 KiB CU):
 *   ring   32 KiB of output history, position p at ring[p & 32767].  Bytes [fp, op) are produced but not yet in the text buffer; they are flushed, coalesced,
 *          as soon as there are INF_SEG (8 KiB) of them, so a write of at most 258 bytes at op never reaches an unflushed slot (8192 + 258 + 258 <= 32768) and
 *          the wave never reads its own global stores back.
 *   win    1 KiB window of the input, position p at win[p & 1023], fetched 512 bytes at a time: the bit buffer is refilled from LDS, not from HBM.
 *   lfast / dfast  the first 10 / 8 bits of the stream -> symbol << 4 | code length (0: longer code, or none); filled by the lanes in parallel, each entry by the
 *          canonical decoder below, which also serves the codes that are longer.
 *   lcount / lsym, dcount / dsym  the canonical codes: codes per length, symbols in code order.  Built by lane 0 from `lens`.
 *
 * Lanes must not rely on running in lock step (the CPU build of the kernels runs them one after the other between two cross-lane operations), so every LDS
 * cell that one lane writes and another reads has a wv_sync() between the two, and every cell that is overwritten has one between its last reader and the
 * writer: before and after a window fetch, before a table build (nobody decodes with the old tables any more) and after it, at the start of a match (the
 * literals lane 0 wrote, the bytes of earlier matches), between the read and the write of each 64-byte round of a match (with distances near 32768 a lane
 * writes the slot its neighbour reads), before a flush.
 *
 * TERMINATION: every iteration of the block loop consumes at least 3 input bits and every iteration of the symbol loop at least 1 (a code longer than the
 * bits that are left is INF_IN_EXHAUSTED), the code-length loop advances by at least one length per iteration, copies are bounded by lengths checked
 * BEFORE the copy; the input holds 8 * in_len bits.  BOUNDS: the input is read at positions < in_len only, the output written at positions < isize only,
 * both checked before the access.
 */
#ifndef MA_INFLATE_CORE_H
#define MA_INFLATE_CORE_H

/* per-member status, in the order of include/mahip.h's MAHIP_BGZF_BAD_BTYPE .. MAHIP_BGZF_CRC */
enum { INF_OK = 0, INF_BAD_BTYPE, INF_STORED_LEN, INF_BAD_LENGTHS, INF_BAD_SYMBOL, INF_DIST_TOO_FAR, INF_OUT_OVERFLOW, INF_IN_EXHAUSTED, INF_OUT_SHORT, INF_CRC };

#define INF_RING 32768u
#define INF_SEG 8192u
#define INF_WIN 1024u
#define INF_FETCH 512u
#define INF_LBITS 10
#define INF_DBITS 8
#define INF_NOSYM 0xffffffffu

/* what the bit reader and the code tables need; the decoders add their output history (InfLds here, GzLds in gzip_core.h) */
struct InfTabs {
	uint8_t win[INF_WIN];
	uint16_t lfast[1 << INF_LBITS], dfast[1 << INF_DBITS];
	uint16_t lcount[16], dcount[16], offs[16];
	uint16_t lsym[288], dsym[32];
	uint8_t lens[320];
	uint32_t brc[4]; /* what lane 0 found while building: lit/len result, its longest code, distance result, its longest code */
};
struct InfLds : InfTabs {
	uint8_t ring[INF_RING];
};

struct InfState {
	const uint8_t *in; uint8_t *out;
	uint32_t in_len, isize;
	uint32_t ip, lp;      /* input: bytes moved into the bit buffer, bytes fetched into the window (ip <= lp <= in_len, lp - ip <= INF_WIN) */
	uint32_t op, fp;      /* output: bytes produced, bytes flushed */
	uint64_t bitbuf; uint32_t bitcnt; /* bits above bitcnt are zero */
	uint32_t err, fixed;  /* fixed: the tables in LDS are those of the fixed code */
	uint32_t nblk[3];     /* deflate blocks by type */
	unsigned lane;
};

/* the code-length alphabet's order (RFC 1951, 3.2.7), five bits an entry */
#define INF_ORD_A (16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55)
#define INF_ORD_B (12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30)

__device__ __forceinline__ void inf_fetch(InfState &s, InfTabs &L)
{
	wv_sync();
	for (uint32_t k = 0; k < INF_FETCH; k += 64) {
		const uint32_t p = s.lp + k + s.lane;
		if (p < s.in_len) L.win[p & (INF_WIN - 1)] = s.in[p];
	}
	s.lp = s.in_len - s.lp < INF_FETCH ? s.in_len : s.lp + INF_FETCH;
	wv_sync();
}

/* afterwards the bit buffer holds at least 32 bits, or all that is left of the input */
__device__ __forceinline__ void inf_refill(InfState &s, InfTabs &L)
{
	if (s.bitcnt >= 32) return;
	if (s.lp - s.ip < 8 && s.lp < s.in_len) inf_fetch(s, L);
	uint32_t n = s.lp - s.ip, w = 0;
	if (n > 4) n = 4;
	for (uint32_t k = 0; k < n; ++k) w |= (uint32_t)L.win[(s.ip + k) & (INF_WIN - 1)] << (8 * k);
	s.bitbuf |= (uint64_t)w << s.bitcnt;
	s.bitcnt += 8 * n; s.ip += n;
}

/* n <= 16 bits, least significant first */
__device__ __forceinline__ uint32_t inf_bits(InfState &s, InfTabs &L, uint32_t n)
{
	inf_refill(s, L);
	if (s.bitcnt < n) { s.err = INF_IN_EXHAUSTED; return 0; }
	const uint32_t v = (uint32_t)s.bitbuf & ((1u << n) - 1u);
	s.bitbuf >>= n; s.bitcnt -= n;
	return v;
}

/* the canonical decoder: the code that `bits` begins with (first bit of the stream = bit 0), if it is at most maxlen long: symbol | length << 16 */
__device__ __forceinline__ uint32_t inf_canon(const uint16_t *count, const uint16_t *symbol, uint32_t bits, uint32_t maxlen)
{
	int code = 0, first = 0, index = 0;
	for (uint32_t len = 1; len <= maxlen; ++len) {
		code |= (int)(bits & 1u); bits >>= 1;
		const int cnt = count[len];
		if (code - cnt < first) return (uint32_t)symbol[index + (code - first)] | len << 16;
		index += cnt; first += cnt; first <<= 1; code <<= 1;
	}
	return INF_NOSYM;
}

__device__ __forceinline__ uint32_t inf_sym(InfState &s, InfTabs &L, const uint16_t *fast, uint32_t fast_bits, const uint16_t *count, const uint16_t *symbol)
{
	inf_refill(s, L);
	const uint32_t b = (uint32_t)s.bitbuf & 0x7fffu, e = fast[b & ((1u << fast_bits) - 1u)];
	uint32_t sym, len;
	if (e) { sym = e >> 4; len = e & 15u; }
	else {
		const uint32_t r = inf_canon(count, symbol, b, 15);
		if (r == INF_NOSYM) { s.err = s.bitcnt < 15 ? INF_IN_EXHAUSTED : INF_BAD_SYMBOL; return 0; }
		sym = r & 0xffffu; len = r >> 16;
	}
	if (len > s.bitcnt) { s.err = INF_IN_EXHAUSTED; return 0; }
	s.bitbuf >>= len; s.bitcnt -= len;
	return sym;
}

/* ONE lane: lens[0 .. n) -> codes per length and symbols in code order.  0: complete, 1: over-subscribed, 2: incomplete; *maxlen: the longest code (0: none) */
__device__ __forceinline__ uint32_t inf_build(InfTabs &L, const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *symbol, uint32_t *maxlen)
{
	for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
	for (uint32_t i = 0; i < n; ++i) ++count[lens[i] & 15u];
	int left = 1;
	uint32_t mx = 0;
	for (uint32_t l = 1; l < 16; ++l) {
		left <<= 1; left -= (int)count[l];
		if (left < 0) return 1;
		if (count[l]) mx = l;
	}
	*maxlen = mx;
	L.offs[1] = 0;
	for (uint32_t l = 1; l < 15; ++l) L.offs[l + 1] = (uint16_t)(L.offs[l] + count[l]);
	for (uint32_t i = 0; i < n; ++i) if (lens[i] & 15u) symbol[L.offs[lens[i] & 15u]++] = (uint16_t)i;
	return left > 0 ? 2u : 0u;
}

/* all lanes: the first fast_bits bits -> symbol << 4 | length */
__device__ __forceinline__ void inf_fill_fast(InfState &s, uint16_t *fast, uint32_t fast_bits, const uint16_t *count, const uint16_t *symbol)
{
	for (uint32_t e = s.lane; e < (1u << fast_bits); e += 64) {
		const uint32_t r = inf_canon(count, symbol, e, fast_bits);
		fast[e] = r == INF_NOSYM ? (uint16_t)0 : (uint16_t)((r & 0xffffu) << 4 | r >> 16);
	}
}

/* lens[0 .. nl) and lens[nl .. nl + nd) are written (and visible): both codes and their tables, with zlib's rules for what is acceptable (inftrees.c: an
 * over-subscribed set never, an incomplete one only when it is a single code of one bit; no distance code at all is fine as long as no match turns up) */
__device__ __forceinline__ void inf_tables(InfState &s, InfTabs &L, uint32_t nl, uint32_t nd)
{
	if (s.lane == 0) {
		uint32_t ml = 0, md = 0;
		L.brc[0] = inf_build(L, L.lens, nl, L.lcount, L.lsym, &ml); L.brc[1] = ml;
		L.brc[2] = inf_build(L, L.lens + nl, nd, L.dcount, L.dsym, &md); L.brc[3] = md;
	}
	wv_sync();
	if (L.brc[0] == 1 || L.brc[2] == 1 || (L.brc[0] == 2 && L.brc[1] != 1) || (L.brc[2] == 2 && L.brc[3] > 1)) { s.err = INF_BAD_LENGTHS; return; }
	inf_fill_fast(s, L.lfast, INF_LBITS, L.lcount, L.lsym);
	inf_fill_fast(s, L.dfast, INF_DBITS, L.dcount, L.dsym);
	wv_sync();
}

__device__ __forceinline__ void inf_flush(InfState &s, InfLds &L)
{
	wv_sync();
	for (uint32_t p = s.fp + s.lane; p < s.op; p += 64) s.out[p] = L.ring[p & (INF_RING - 1)];
	s.fp = s.op;
}

__device__ __forceinline__ void inf_stored(InfState &s, InfLds &L)
{
	const uint32_t drop = s.bitcnt & 7u; /* to the next byte border of the input */
	s.bitbuf >>= drop; s.bitcnt -= drop;
	const uint32_t len = inf_bits(s, L, 16), nlen = inf_bits(s, L, 16);
	if (s.err) return;
	if (len != (~nlen & 0xffffu)) { s.err = INF_STORED_LEN; return; }
	s.ip -= s.bitcnt >> 3; s.bitbuf = 0; s.bitcnt = 0; /* whole bytes go back: the copy takes them from the input itself */
	if (len > s.in_len - s.ip) { s.err = INF_IN_EXHAUSTED; return; }
	if (len > s.isize - s.op) { s.err = INF_OUT_OVERFLOW; return; }
	for (uint32_t done = 0; done < len; done += 256) {
		const uint32_t n = len - done < 256 ? len - done : 256;
		for (uint32_t k = s.lane; k < n; k += 64) L.ring[(s.op + k) & (INF_RING - 1)] = s.in[s.ip + done + k];
		s.op += n;
		if (s.op - s.fp >= INF_SEG) inf_flush(s, L);
	}
	s.ip += len;
	if (s.lp < s.ip) s.lp = s.ip; /* the window starts again behind the block */
}

__device__ __forceinline__ void inf_fixed(InfState &s, InfTabs &L)
{
	if (s.fixed) return;
	for (uint32_t i = s.lane; i < 320; i += 64) L.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5; /* 288 literal/length codes, 32 distance codes of 5 bits */
	wv_sync();
	inf_tables(s, L, 288, 32);
	s.fixed = 1;
}

__device__ __forceinline__ void inf_dynamic(InfState &s, InfTabs &L)
{
	s.fixed = 0;
	const uint32_t hlit = inf_bits(s, L, 5) + 257, hdist = inf_bits(s, L, 5) + 1, hclen = inf_bits(s, L, 4) + 4;
	if (s.err) return;
	if (hlit > 286 || hdist > 30) { s.err = INF_BAD_LENGTHS; return; }
	if (s.lane < 19) L.lens[s.lane] = 0;
	wv_sync();
	for (uint32_t k = 0; k < hclen; ++k) {
		const uint32_t v = inf_bits(s, L, 3), o = (uint32_t)((k < 12 ? INF_ORD_A >> (5 * k) : INF_ORD_B >> (5 * (k - 12))) & 31u);
		if (s.lane == 0) L.lens[o] = (uint8_t)v;
	}
	if (s.err) return;
	wv_sync();
	if (s.lane == 0) { uint32_t mc = 0; L.brc[0] = inf_build(L, L.lens, 19, L.dcount, L.dsym, &mc); } /* the code-length code borrows the distance code's arrays */
	wv_sync();
	if (L.brc[0] != 0) { s.err = INF_BAD_LENGTHS; return; }
	/* HLIT + HDIST lengths are ONE sequence: a repeat may run from the literal/length lengths into the distance lengths */
	const uint32_t total = hlit + hdist;
	uint32_t prev = 0;
	for (uint32_t i = 0; i < total;) {
		inf_refill(s, L);
		const uint32_t r = inf_canon(L.dcount, L.dsym, (uint32_t)s.bitbuf & 0x7fu, 7);
		if (r == INF_NOSYM) { s.err = s.bitcnt < 7 ? INF_IN_EXHAUSTED : INF_BAD_LENGTHS; return; }
		if ((r >> 16) > s.bitcnt) { s.err = INF_IN_EXHAUSTED; return; }
		s.bitbuf >>= (r >> 16); s.bitcnt -= (r >> 16);
		const uint32_t sym = r & 0xffffu;
		uint32_t rep = 1, val = sym;
		if (sym == 16) { if (i == 0) { s.err = INF_BAD_LENGTHS; return; } rep = 3 + inf_bits(s, L, 2); val = prev; }
		else if (sym == 17) { rep = 3 + inf_bits(s, L, 3); val = 0; }
		else if (sym == 18) { rep = 11 + inf_bits(s, L, 7); val = 0; }
		if (s.err) return;
		if (rep > total - i) { s.err = INF_BAD_LENGTHS; return; }
		if (s.lane == 0) for (uint32_t k = 0; k < rep; ++k) L.lens[i + k] = (uint8_t)val;
		i += rep; prev = val;
	}
	wv_sync();
	if (L.lens[256] == 0) { s.err = INF_BAD_LENGTHS; return; } /* no end-of-block code */
	inf_tables(s, L, hlit, hdist);
}

/* literals, matches, end of block */
__device__ __forceinline__ void inf_codes(InfState &s, InfLds &L)
{
	for (;;) {
		uint32_t sym = inf_sym(s, L, L.lfast, INF_LBITS, L.lcount, L.lsym);
		if (s.err) return;
		if (sym < 256) {
			if (s.op >= s.isize) { s.err = INF_OUT_OVERFLOW; return; }
			if (s.lane == 0) L.ring[s.op & (INF_RING - 1)] = (uint8_t)sym;
			++s.op;
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
			if (dist > s.op) { s.err = INF_DIST_TOO_FAR; return; } /* members are independent: nothing in front of this one's output */
			if (len > s.isize - s.op) { s.err = INF_OUT_OVERFLOW; return; }
			wv_sync();
			for (uint32_t r = 0; r < len; r += 64) { /* lane i copies byte r + i; a match that overlaps itself repeats its first `dist` bytes */
				const uint32_t k = r + s.lane;
				uint8_t v = 0;
				if (k < len) v = L.ring[(s.op - dist + (k < dist ? k : k % dist)) & (INF_RING - 1)];
				wv_sync();
				if (k < len) L.ring[(s.op + k) & (INF_RING - 1)] = v;
			}
			s.op += len;
		}
		if (s.op - s.fp >= INF_SEG) inf_flush(s, L);
	}
}

/* the whole wave; returns the status (the same in every lane) */
__device__ __forceinline__ uint32_t inf_member(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, InfLds &L, unsigned lane, uint32_t nblk[3])
{
	InfState s;
	s.in = in; s.out = out; s.in_len = in_len; s.isize = isize;
	s.ip = s.lp = s.op = s.fp = 0; s.bitbuf = 0; s.bitcnt = 0; s.err = INF_OK; s.fixed = 0; s.lane = lane;
	s.nblk[0] = s.nblk[1] = s.nblk[2] = 0;
	uint32_t last;
	do {
		last = inf_bits(s, L, 1);
		const uint32_t type = inf_bits(s, L, 2);
		if (s.err) break;
		if (type == 3) { s.err = INF_BAD_BTYPE; break; }
		s.nblk[0] += type == 0; s.nblk[1] += type == 1; s.nblk[2] += type == 2;
		wv_sync(); /* nobody decodes with the tables of the block before any more */
		if (type == 0) inf_stored(s, L);
		else {
			if (type == 1) inf_fixed(s, L); else inf_dynamic(s, L);
			if (!s.err) inf_codes(s, L);
		}
	} while (!last && !s.err);
	if (!s.err && s.op != s.isize) s.err = INF_OUT_SHORT;
	inf_flush(s, L);
	nblk[0] = s.nblk[0]; nblk[1] = s.nblk[1]; nblk[2] = s.nblk[2];
	return s.err;
}

/* ---- CRC-32 (the gzip polynomial, bit-reflected: x^k for k < 32 is 1 << (31 - k)) ---- */
#define INF_CRC_POLY 0xedb88320u
/* a(x) * b(x) mod P */
__device__ __forceinline__ uint32_t inf_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = b & 1u ? (b >> 1) ^ INF_CRC_POLY : b >> 1;
	}
	return p;
}
/* x^(8 n) mod P: the factor that moves a CRC in front of n more bytes (crc(A B) = crc(A) * x^(8 |B|) ^ crc(B)) */
__device__ __forceinline__ uint32_t inf_xpow8(uint32_t n)
{
	uint32_t p = 0x80000000u, sq = 0x00800000u; /* x^0, x^8 */
	for (; n; n >>= 1) {
		if (n & 1u) p = inf_mulmod(p, sq);
		sq = inf_mulmod(sq, sq);
	}
	return p;
}
/* the same for a text of more than 4 GiB */
__device__ __forceinline__ uint32_t inf_xpow8_64(uint64_t n)
{
	uint32_t p = 0x80000000u, sq = 0x00800000u;
	for (; n; n >>= 1) {
		if (n & 1u) p = inf_mulmod(p, sq);
		sq = inf_mulmod(sq, sq);
	}
	return p;
}
#endif
