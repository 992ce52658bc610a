/* text_core.h -- the lines of the three record dumps, written once for device (HIP) and host (unit tests).
 *
 *   tc_line_paf : reference main.c:21-30 (print_hits)   "%s:%d-%d\t%d\t%d\t%d\t%c\t%s:%d-%d\t%d\t%d\t%d\t%d\t%d\t255\n"
 *   tc_line_sg  : reference asm.c:41-55  (ma_sg_print)  "L\t%s:%d-%d\t%c\t%s:%d-%d\t%c\t%d:\tL1:i:%d\n"   (without sub: "L\t%s\t%c\t%s\t%c\t%d:\tL1:i:%d\n")
 *   tc_line_bed : reference main.c:13-19 (print_subs)   "%s\t%d\t%d\n", nothing for a read that is del or has s == e
 *
 * Every routine writes through an emitter.  An emitter without a buffer only counts: that is the length pass; with a buffer it stores: that is the
 * write pass.  Both passes run the same routine, so the length of a line and its bytes cannot disagree.
 *
 * %d takes an int.  The reference hands it uint32_t values in several places (the low word of qns, qe, ts, te, sub.e, e - s, the arc length): they
 * print as the int with the same bits, negative above 2^31 - 1.  The 31-bit bit-fields (sub.s, ml, bl, ol) promote to int and are never negative;
 * sub.s + 1 is an int addition, so sub.s = 2^31 - 1 is undefined in the reference and not supported here.
 */
#ifndef MA_TEXT_CORE_H
#define MA_TEXT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TC_HD __host__ __device__ __forceinline__
#else
#define TC_HD static inline
#endif

#define TC_KIND_PAF 1
#define TC_KIND_SG  2
#define TC_KIND_BED 3

/* the longest line of each kind without its names: 11 bytes per %d ("-2147483648"), the literals counted one by one */
#define TC_FIXED_PAF (2 * (1 + 11 + 1 + 11) + 9 * 11 + 1 + 11 + 4)
#define TC_FIXED_SG  (2 + 2 * (1 + 11 + 1 + 11) + 4 + 2 + 11 + 7 + 11 + 1)
#define TC_FIXED_BED (1 + 11 + 1 + 11 + 1)

typedef struct { char *p; uint32_t n; } tc_emit_t; /* p == 0: count only */

/* names: the bytes of name i are blob[off[i] .. off[i + 1]) (no terminator) */
typedef struct { const char *blob; const uint64_t *off; } tc_names_t;

TC_HD void tc_chr(tc_emit_t *e, char c) { if (e->p) e->p[e->n] = c; ++e->n; }

TC_HD uint32_t tc_ndig(uint32_t x) /* decimal digits of x: nine compares, no loop */
{
	return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) + (x >= 100000000u) + (x >= 1000000000u);
}

/* the five decimal digits of v < 100000, most significant first: v / 10^4 as a 32.32 fixed-point number (429497 = ceil(2^32 / 10^4): the excess, below
 * 100000 * 0.28 / 2^32 = 6.4e-6, stays under one unit of the last digit, 1e-4), then the fraction times ten, four times.  No division.
 * (tests/text_core_host.c compares every v < 100000 with the quotients.) */
TC_HD void tc_dig5(uint32_t v, uint32_t d[5])
{
	uint64_t t = (uint64_t)v * 429497ull;
	d[0] = (uint32_t)(t >> 32); t = (uint64_t)(uint32_t)t * 10ull;
	d[1] = (uint32_t)(t >> 32); t = (uint64_t)(uint32_t)t * 10ull;
	d[2] = (uint32_t)(t >> 32); t = (uint64_t)(uint32_t)t * 10ull;
	d[3] = (uint32_t)(t >> 32); t = (uint64_t)(uint32_t)t * 10ull;
	d[4] = (uint32_t)(t >> 32);
}

TC_HD void tc_int(tc_emit_t *e, int32_t v) /* %d */
{
	const uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v, n = tc_ndig(u);
	if (e->p) {
		char *q = e->p + e->n;
		const uint32_t hi = u / 100000u, lo = u - hi * 100000u; /* one multiply-high */
		uint32_t a[5], b[5];
		tc_dig5(hi, a); tc_dig5(lo, b);
		if (v < 0) *q++ = '-';
		/* digit k of ten is printed when the number has more than 9 - k digits; the indices are constants, so the digits stay in registers */
		if (n > 9) *q++ = (char)('0' + a[0]);
		if (n > 8) *q++ = (char)('0' + a[1]);
		if (n > 7) *q++ = (char)('0' + a[2]);
		if (n > 6) *q++ = (char)('0' + a[3]);
		if (n > 5) *q++ = (char)('0' + a[4]);
		if (n > 4) *q++ = (char)('0' + b[0]);
		if (n > 3) *q++ = (char)('0' + b[1]);
		if (n > 2) *q++ = (char)('0' + b[2]);
		if (n > 1) *q++ = (char)('0' + b[3]);
		*q = (char)('0' + b[4]);
	}
	e->n += n + (v < 0 ? 1u : 0u);
}

TC_HD void tc_name(tc_emit_t *e, const tc_names_t *nm, uint32_t id)
{
	const uint64_t a = nm->off[id], b = nm->off[id + 1];
	const uint32_t l = (uint32_t)(b - a);
	if (e->p) {
		const char *s = nm->blob + a;
		char *q = e->p + e->n;
		uint32_t k;
		for (k = 0; k < l; ++k) q[k] = s[k];
	}
	e->n += l;
}

/* "name:s+1-e", or the bare name without sub.  sub: two words per read, word 0 = s | del << 31, word 1 = e (ma_sub_t) */
TC_HD void tc_read(tc_emit_t *e, const tc_names_t *nm, const uint32_t *sub, uint32_t id)
{
	tc_name(e, nm, id);
	if (sub) {
		tc_chr(e, ':'); tc_int(e, (int32_t)(sub[2 * (uint64_t)id] & 0x7fffffffu) + 1);
		tc_chr(e, '-'); tc_int(e, (int32_t)sub[2 * (uint64_t)id + 1]);
	}
}

/* h: the eight words of a ma_hit_t (qns low = query start, qns high = query id, qe, tn, ts, te, ml | rev << 31, bl | del << 31) */
TC_HD void tc_line_paf(tc_emit_t *e, const uint32_t *h, const tc_names_t *nm, const uint32_t *sub)
{
	const uint32_t q = h[1], t = h[3];
	tc_read(e, nm, sub, q); tc_chr(e, '\t');
	tc_int(e, (int32_t)(sub[2 * (uint64_t)q + 1] - (sub[2 * (uint64_t)q] & 0x7fffffffu))); tc_chr(e, '\t');
	tc_int(e, (int32_t)h[0]); tc_chr(e, '\t');
	tc_int(e, (int32_t)h[2]); tc_chr(e, '\t');
	tc_chr(e, (h[6] >> 31) ? '-' : '+'); tc_chr(e, '\t');
	tc_read(e, nm, sub, t); tc_chr(e, '\t');
	tc_int(e, (int32_t)(sub[2 * (uint64_t)t + 1] - (sub[2 * (uint64_t)t] & 0x7fffffffu))); tc_chr(e, '\t');
	tc_int(e, (int32_t)h[4]); tc_chr(e, '\t');
	tc_int(e, (int32_t)h[5]); tc_chr(e, '\t');
	tc_int(e, (int32_t)(h[6] & 0x7fffffffu)); tc_chr(e, '\t');
	tc_int(e, (int32_t)(h[7] & 0x7fffffffu));
	tc_chr(e, '\t'); tc_chr(e, '2'); tc_chr(e, '5'); tc_chr(e, '5'); tc_chr(e, '\n');
}

/* a: the four words of an asg_arc_t (ul low = arc length, ul high = u, v, ol | del << 31); sub may be 0 */
TC_HD void tc_line_sg(tc_emit_t *e, const uint32_t *a, const tc_names_t *nm, const uint32_t *sub)
{
	tc_chr(e, 'L'); tc_chr(e, '\t');
	tc_read(e, nm, sub, a[1] >> 1); tc_chr(e, '\t'); tc_chr(e, (a[1] & 1u) ? '-' : '+'); tc_chr(e, '\t');
	tc_read(e, nm, sub, a[2] >> 1); tc_chr(e, '\t'); tc_chr(e, (a[2] & 1u) ? '-' : '+'); tc_chr(e, '\t');
	tc_int(e, (int32_t)(a[3] & 0x7fffffffu));
	tc_chr(e, ':'); tc_chr(e, '\t'); tc_chr(e, 'L'); tc_chr(e, '1'); tc_chr(e, ':'); tc_chr(e, 'i'); tc_chr(e, ':');
	tc_int(e, (int32_t)a[0]); tc_chr(e, '\n');
}

/* read id of the dictionary the names describe; del: one byte per read, or 0 when no read is deleted */
TC_HD void tc_line_bed(tc_emit_t *e, uint32_t id, const tc_names_t *nm, const uint32_t *sub, const uint8_t *del)
{
	const uint32_t s = sub[2 * (uint64_t)id] & 0x7fffffffu, en = sub[2 * (uint64_t)id + 1];
	if ((del && del[id]) || s == en) return;
	tc_name(e, nm, id); tc_chr(e, '\t'); tc_int(e, (int32_t)s); tc_chr(e, '\t'); tc_int(e, (int32_t)en); tc_chr(e, '\n');
}

/* record r of a dump of the given kind; rec: the records (paf: 8 words each, sg: 4 words each, bed: unused) */
TC_HD void tc_line(tc_emit_t *e, int kind, uint64_t r, const uint32_t *rec, const tc_names_t *nm, const uint32_t *sub, const uint8_t *del)
{
	if (kind == TC_KIND_PAF) tc_line_paf(e, rec + 8 * r, nm, sub);
	else if (kind == TC_KIND_SG) tc_line_sg(e, rec + 4 * r, nm, sub);
	else tc_line_bed(e, (uint32_t)r, nm, sub, del);
}

#endif
