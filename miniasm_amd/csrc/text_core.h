/* text_core.h -- the lines of the three record dumps and of the unitig GFA, written once for device (HIP) and host (unit tests).
 *
 *   tc_line_paf : reference main.c:21-30 (print_hits)   "%s:%d-%d\t%d\t%d\t%d\t%c\t%s:%d-%d\t%d\t%d\t%d\t%d\t%d\t255\n"
 *   tc_line_sg  : reference asm.c:41-55  (ma_sg_print)  "L\t%s:%d-%d\t%c\t%s:%d-%d\t%c\t%d:\tL1:i:%d\n"   (without sub: "L\t%s\t%c\t%s\t%c\t%d:\tL1:i:%d\n")
 *   tc_line_bed : reference main.c:13-19 (print_subs)   "%s\t%d\t%d\n", nothing for a read that is del or has s == e
 *   tc_line_ug  : reference asm.c:77-116 (ma_ug_print)  the S / L / a / x lines of -p ug, one RECORD of its record space at a time (tc_ug_t below)
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
#define TC_KIND_UG  4

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

TC_HD void tc_udec(tc_emit_t *e, uint32_t u) /* the decimal digits of u */
{
	const uint32_t n = tc_ndig(u);
	if (e->p) {
		char *q = e->p + e->n;
		const uint32_t hi = u / 100000u, lo = u - hi * 100000u; /* one multiply-high */
		uint32_t a[5], b[5];
		tc_dig5(hi, a); tc_dig5(lo, b);
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
	e->n += n;
}

TC_HD void tc_int(tc_emit_t *e, int32_t v) /* %d */
{
	if (v < 0) tc_chr(e, '-');
	tc_udec(e, v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
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

/* ---- the unitig GFA (reference asm.c:77-116, ma_ug_print): three blocks -- units (S, circularising L, a), links (L), summary (x) ---- */

/* "utg%.6d%c": the reference hands i + 1 (a uint32_t) to %d; the precision pads the DIGITS to six, a sign stands in front of them */
TC_HD void tc_utg(tc_emit_t *e, uint32_t id1, int circ)
{
	const int32_t v = (int32_t)id1;
	const uint32_t u = v < 0 ? 0u - id1 : id1;
	uint32_t k;
	tc_chr(e, 'u'); tc_chr(e, 't'); tc_chr(e, 'g');
	if (v < 0) tc_chr(e, '-');
	for (k = tc_ndig(u); k < 6u; ++k) tc_chr(e, '0');
	tc_udec(e, u);
	tc_chr(e, circ ? 'c' : 'l');
}

/* "L\t%s\t+\t%s\t+\t0M\n" and the '-' twin: the circularising links of a circular unitig (asm.c:85-88) */
TC_HD void tc_ug_circ(tc_emit_t *e, uint32_t id1)
{
	int j;
	for (j = 0; j < 2; ++j) {
		const char c = j ? '-' : '+';
		tc_chr(e, 'L'); tc_chr(e, '\t'); tc_utg(e, id1, 1); tc_chr(e, '\t'); tc_chr(e, c); tc_chr(e, '\t');
		tc_utg(e, id1, 1); tc_chr(e, '\t'); tc_chr(e, c); tc_chr(e, '\t'); tc_chr(e, '0'); tc_chr(e, 'M'); tc_chr(e, '\n');
	}
}

/* the S line in its pieces: head "S\t<utg>\t", the sequence (or "*"), tail "\tLN:i:%d\n" and, for a circular unitig, the circularising links */
TC_HD void tc_ug_s_head(tc_emit_t *e, uint32_t id1, int circ) { tc_chr(e, 'S'); tc_chr(e, '\t'); tc_utg(e, id1, circ); tc_chr(e, '\t'); }
TC_HD void tc_ug_s_tail(tc_emit_t *e, uint32_t id1, int circ, uint32_t len)
{
	tc_chr(e, '\t'); tc_chr(e, 'L'); tc_chr(e, 'N'); tc_chr(e, ':'); tc_chr(e, 'i'); tc_chr(e, ':'); tc_int(e, (int32_t)len); tc_chr(e, '\n');
	if (circ) tc_ug_circ(e, id1);
}
TC_HD void tc_ug_s(tc_emit_t *e, uint32_t id1, int circ, uint32_t len) { tc_ug_s_head(e, id1, circ); tc_chr(e, '*'); tc_ug_s_tail(e, id1, circ, len); }

/* n bases of a sequence: no formatting, the length is arithmetic */
TC_HD void tc_bytes(tc_emit_t *e, const char *s, uint32_t n)
{
	if (e->p) {
		char *q = e->p + e->n;
		uint32_t k;
		for (k = 0; k < n; ++k) q[k] = s[k];
	}
	e->n += n;
}

/* "a\t%s\t%d\t%s:%d-%d\t%c\t%d\n": m = the member word (vertex << 32 | length to the next read), l = the offset of the read on the unitig */
TC_HD void tc_ug_a(tc_emit_t *e, uint32_t id1, int circ, uint32_t l, uint64_t m, const tc_names_t *nm, const uint32_t *sub)
{
	tc_chr(e, 'a'); tc_chr(e, '\t'); tc_utg(e, id1, circ); tc_chr(e, '\t'); tc_int(e, (int32_t)l); tc_chr(e, '\t');
	tc_read(e, nm, sub, (uint32_t)(m >> 33)); tc_chr(e, '\t'); tc_chr(e, (m >> 32 & 1u) ? '-' : '+'); tc_chr(e, '\t');
	tc_int(e, (int32_t)(uint32_t)m); tc_chr(e, '\n');
}

/* "L\tutg%.6d%c\t%c\tutg%.6d%c\t%c\t%dM\tSD:i:%d\n": a = the four words of a unitig arc, cu / cv = the circular flags of its two unitigs */
TC_HD void tc_ug_l(tc_emit_t *e, const uint32_t *a, int cu, int cv)
{
	tc_chr(e, 'L'); tc_chr(e, '\t');
	tc_utg(e, (a[1] >> 1) + 1u, cu); tc_chr(e, '\t'); tc_chr(e, (a[1] & 1u) ? '-' : '+'); tc_chr(e, '\t');
	tc_utg(e, (a[2] >> 1) + 1u, cv); tc_chr(e, '\t'); tc_chr(e, (a[2] & 1u) ? '-' : '+'); tc_chr(e, '\t');
	tc_int(e, (int32_t)(a[3] & 0x7fffffffu));
	tc_chr(e, 'M'); tc_chr(e, '\t'); tc_chr(e, 'S'); tc_chr(e, 'D'); tc_chr(e, ':'); tc_chr(e, 'i'); tc_chr(e, ':');
	tc_int(e, (int32_t)a[0]); tc_chr(e, '\n');
}

/* "x\tutg%.6dc\t%d\t%d\n" (start == 0xffffffff: circular) or "x\tutg%.6dl\t%d\t%d\t%d\t%d\t%s:%d-%d\t%c\t%s:%d-%d\t%c\n"; c0 / c1 = arcs leaving end 0 / 1 */
TC_HD void tc_ug_x(tc_emit_t *e, uint32_t id1, uint32_t len, uint32_t n, uint32_t start, uint32_t end, uint32_t c0, uint32_t c1, const tc_names_t *nm, const uint32_t *sub)
{
	const int circ = start == 0xffffffffu;
	tc_chr(e, 'x'); tc_chr(e, '\t'); tc_utg(e, id1, circ); tc_chr(e, '\t'); tc_int(e, (int32_t)len); tc_chr(e, '\t'); tc_int(e, (int32_t)n);
	if (!circ) {
		tc_chr(e, '\t'); tc_int(e, (int32_t)c1); tc_chr(e, '\t'); tc_int(e, (int32_t)c0); tc_chr(e, '\t');
		tc_read(e, nm, sub, start >> 1); tc_chr(e, '\t'); tc_chr(e, (start & 1u) ? '-' : '+'); tc_chr(e, '\t');
		tc_read(e, nm, sub, end >> 1); tc_chr(e, '\t'); tc_chr(e, (end & 1u) ? '-' : '+');
	}
	tc_chr(e, '\n');
}

/* The unitigs as dense arrays, and the record space of the GFA over them.  Units block: unitig i owns the records [rbase[i], rbase[i + 1]) --
 *   without sequences (arena == 0):  its S line with the circularising links behind it, then one record per member;
 *   with sequences:                  the head of the S line, ceil(u_len / chunk) chunk records of `chunk` bases each (the last one shorter), the tail, the members.
 * Behind them n_links link records and U summary records.  rbase rises strictly (every unitig has its S line), so a record finds its unitig by bisection.
 * moff[i] = first member of unitig i in mem; mscan = the exclusive prefix sum (mod 2^32) of the members' low words over ALL members: a member's offset on its
 * unitig is mscan[m] - mscan[moff[i]], the reference's uint32_t l.  cnt[2 i + e] = arcs that leave end e of unitig i (asg_arc_n).  uoff[i] = where unitig i's
 * bases start in arena (host/unitig_gfa.c: ma_ug_seq lays the strings back to back with one spare byte behind each). */
typedef struct {
	uint32_t U, n_links, chunk;
	uint64_t n_unit_rec;
	const uint32_t *u_n, *u_len, *u_start, *u_end, *moff, *rbase, *mscan, *links, *cnt;
	const uint64_t *mem, *uoff;
	const char *arena;
} tc_ug_t;

#define TC_UTG_MAX (3 + 11 + 1) /* "utg", a %d, the l / c letter */
/* the longest record of the unitig GFA without its names: the linear x line (two reads, each with ":%d-%d"), which outgrows the S line with both circularising
 * links (2 + UTG + 1 + 1 + 6 + 11 + 1 + 2 * (2 + 2 * UTG + 3 + 6) = 119), the a line (69) and the L line (68) */
#define TC_FIXED_UG_S (2 + TC_UTG_MAX + 1 + 1 + 6 + 11 + 1 + 2 * (2 + TC_UTG_MAX + 3 + TC_UTG_MAX + 6))
#define TC_FIXED_UG_A (2 + TC_UTG_MAX + 1 + 11 + 1 + (1 + 11 + 1 + 11) + 1 + 1 + 1 + 11 + 1)
#define TC_FIXED_UG_L (2 + 2 * (TC_UTG_MAX + 1 + 1 + 1) + 11 + 7 + 11 + 1)
#define TC_FIXED_UG_X (2 + TC_UTG_MAX + 4 * (1 + 11) + 2 * (1 + (1 + 11 + 1 + 11) + 1 + 1) + 1)
#define TC_FIXED_UG   TC_FIXED_UG_X

/* where member m starts on the unitig whose first member is m0: the reference's uint32_t l, mod 2^32 -- what the `a` lines print (asm.c:100-103) and where the
 * member's bases go (asm.c:252-258; csrc/useq.hip: the placement plan) */
TC_HD uint32_t tc_ug_member_start(const uint32_t *mscan, uint32_t m0, uint32_t m) { return mscan[m] - mscan[m0]; }

/* record r of the unitig GFA; returns the '\n' bytes it holds */
TC_HD uint32_t tc_line_ug(tc_emit_t *e, const tc_ug_t *g, uint64_t r, const tc_names_t *nm, const uint32_t *sub)
{
	if (r < g->n_unit_rec) {
		uint32_t lo = 0, hi = g->U, i, k, len, circ;
		while (hi - lo > 1u) { /* the last unitig whose first record is not behind r */
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if ((uint64_t)g->rbase[mid] <= r) lo = mid; else hi = mid;
		}
		i = lo; k = (uint32_t)(r - g->rbase[i]); len = g->u_len[i]; circ = g->u_start[i] == 0xffffffffu;
		if (g->arena) {
			const uint32_t nch = len / g->chunk + (len % g->chunk != 0);
			if (k == 0) { tc_ug_s_head(e, i + 1u, (int)circ); return 0; }
			if (k <= nch) {
				const uint32_t at = (k - 1u) * g->chunk;
				tc_bytes(e, g->arena + g->uoff[i] + at, len - at < g->chunk ? len - at : g->chunk);
				return 0;
			}
			if (k == nch + 1u) { tc_ug_s_tail(e, i + 1u, (int)circ, len); return circ ? 3u : 1u; }
			k -= nch + 1u;
		} else if (k == 0) { tc_ug_s(e, i + 1u, (int)circ, len); return circ ? 3u : 1u; }
		{
			const uint32_t m0 = g->moff[i], m = m0 + (k - 1u);
			tc_ug_a(e, i + 1u, (int)circ, tc_ug_member_start(g->mscan, m0, m), g->mem[m], nm, sub);
		}
		return 1;
	}
	r -= g->n_unit_rec;
	if (r < g->n_links) {
		const uint32_t *a = g->links + 4 * r;
		tc_ug_l(e, a, g->u_start[a[1] >> 1] == 0xffffffffu, g->u_start[a[2] >> 1] == 0xffffffffu);
		return 1;
	}
	r -= g->n_links;
	tc_ug_x(e, (uint32_t)r + 1u, g->u_len[r], g->u_n[r], g->u_start[r], g->u_end[r], g->cnt[2 * r], g->cnt[2 * r + 1], nm, sub);
	return 1;
}

/* record r of a dump of the given kind; rec: the records (paf: 8 words each, sg: 4 words each, bed: unused) */
TC_HD void tc_line(tc_emit_t *e, int kind, uint64_t r, const uint32_t *rec, const tc_names_t *nm, const uint32_t *sub, const uint8_t *del)
{
	if (kind == TC_KIND_PAF) tc_line_paf(e, rec + 8 * r, nm, sub);
	else if (kind == TC_KIND_SG) tc_line_sg(e, rec + 4 * r, nm, sub);
	else tc_line_bed(e, (uint32_t)r, nm, sub, del);
}

#endif
