/* text_core.h's unitig-GFA routines compiled for the host, each next to the reference's own fprintf call (asm.c:77-116, format strings and argument types
 * copied: a uint32_t handed to %d, a 31-bit bit-field promoted to int): tests/test_text_ug_core_cpu.py walks the value edges through both.
 * Every tu_* function runs the length pass and the write pass of the routine, writes the routine's bytes to `out` (NUL-terminated, cap bytes) and returns
 * their length when they equal snprintf's, -1 when the two passes disagree, -2 when the text differs from snprintf's, -3 when cap is too small. */
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "text_core.h"

typedef struct { uint32_t s:31, del:1, e; } sub_t;            /* miniasm.h: ma_sub_t */
typedef struct { uint64_t ul; uint32_t v; uint32_t ol:31, del:1; } arc_t; /* asg.h: asg_arc_t */

static long verdict(const tc_emit_t *cnt, const tc_emit_t *st, char *out, size_t cap, const char *ref, int ref_len)
{
	if (st->n != cnt->n) return -1;
	if (st->n + 1 > cap) return -3;
	out[st->n] = 0;
	if (ref_len < 0 || (uint32_t)ref_len != st->n || memcmp(out, ref, st->n) != 0) return -2;
	return (long)st->n;
}

#define REF_CAP 70000
static char g_ref[REF_CAP];

long tu_utg(uint32_t id1, int circ, char *out, size_t cap)
{
	tc_emit_t cnt = {0, 0}, st = {out, 0};
	int n = snprintf(g_ref, REF_CAP, "utg%.6d%c", id1, "lc"[circ]);
	tc_utg(&cnt, id1, circ);
	if (cnt.n + 1 > cap) return -3;
	tc_utg(&st, id1, circ);
	return verdict(&cnt, &st, out, cap, g_ref, n);
}

/* the S line and what follows it for a circular unitig; seq == 0: "*"; otherwise head + bases + tail, as the device cuts it */
long tu_s(uint32_t id1, int circ, uint32_t len, const char *seq, char *out, size_t cap)
{
	tc_emit_t cnt = {0, 0}, st = {out, 0};
	char name[32];
	int n;
	sprintf(name, "utg%.6d%c", id1, "lc"[circ]);
	n = snprintf(g_ref, REF_CAP, "S\t%s\t%s\tLN:i:%d\n", name, seq ? seq : "*", len);
	if (circ) {
		n += snprintf(g_ref + n, REF_CAP - n, "L\t%s\t+\t%s\t+\t0M\n", name, name);
		n += snprintf(g_ref + n, REF_CAP - n, "L\t%s\t-\t%s\t-\t0M\n", name, name);
	}
	if (seq) { tc_ug_s_head(&cnt, id1, circ); tc_bytes(&cnt, seq, (uint32_t)strlen(seq)); tc_ug_s_tail(&cnt, id1, circ, len); }
	else tc_ug_s(&cnt, id1, circ, len);
	if (cnt.n + 1 > cap) return -3;
	if (seq) { tc_ug_s_head(&st, id1, circ); tc_bytes(&st, seq, (uint32_t)strlen(seq)); tc_ug_s_tail(&st, id1, circ, len); }
	else tc_ug_s(&st, id1, circ, len);
	return verdict(&cnt, &st, out, cap, g_ref, n);
}

/* an a line of read 0 (rname); m: strand << 32 | low word */
long tu_a(uint32_t id1, int circ, uint32_t l, uint64_t m, const char *rname, int have_sub, uint32_t s, uint32_t e, char *out, size_t cap)
{
	tc_emit_t cnt = {0, 0}, st = {out, 0};
	const uint64_t off[2] = {0, strlen(rname)};
	const tc_names_t nm = {rname, off};
	const uint32_t subw[2] = {s, e};
	sub_t sub;
	char name[32];
	int n;
	sub.s = s; sub.del = 0; sub.e = e;
	sprintf(name, "utg%.6d%c", id1, "lc"[circ]);
	if (have_sub) n = snprintf(g_ref, REF_CAP, "a\t%s\t%d\t%s:%d-%d\t%c\t%d\n", name, l, rname, sub.s + 1, sub.e, "+-"[m >> 32 & 1], (uint32_t)m);
	else n = snprintf(g_ref, REF_CAP, "a\t%s\t%d\t%s\t%c\t%d\n", name, l, rname, "+-"[m >> 32 & 1], (uint32_t)m);
	tc_ug_a(&cnt, id1, circ, l, m, &nm, have_sub ? subw : 0);
	if (cnt.n + 1 > cap) return -3;
	tc_ug_a(&st, id1, circ, l, m, &nm, have_sub ? subw : 0);
	return verdict(&cnt, &st, out, cap, g_ref, n);
}

long tu_l(uint32_t u, uint32_t v, uint32_t ol, uint32_t len, int cu, int cv, char *out, size_t cap)
{
	tc_emit_t cnt = {0, 0}, st = {out, 0};
	arc_t a;
	uint32_t w[4];
	int n;
	a.ul = (uint64_t)u << 32 | len; a.v = v; a.ol = ol; a.del = 0;
	n = snprintf(g_ref, REF_CAP, "L\tutg%.6d%c\t%c\tutg%.6d%c\t%c\t%dM\tSD:i:%d\n", (u >> 1) + 1, "lc"[cu], "+-"[u & 1], (v >> 1) + 1, "lc"[cv], "+-"[v & 1], a.ol, (uint32_t)a.ul);
	w[0] = len; w[1] = u; w[2] = v; w[3] = ol;
	tc_ug_l(&cnt, w, cu, cv);
	if (cnt.n + 1 > cap) return -3;
	tc_ug_l(&st, w, cu, cv);
	return verdict(&cnt, &st, out, cap, g_ref, n);
}

/* an x line; the reads are 0 (name0) and 1 (name1), start / end = read << 1 | strand, or both 0xffffffff; sw: s0, e0, s1, e1 */
long tu_x(uint32_t id1, uint32_t len, uint32_t n_reads, uint32_t start, uint32_t end, uint32_t c0, uint32_t c1, const char *name0, const char *name1, int have_sub, const uint32_t *sw,
          char *out, size_t cap)
{
	tc_emit_t cnt = {0, 0}, st = {out, 0};
	static char blob[2 * REF_CAP / 4];
	uint64_t off[3];
	tc_names_t nm = {blob, off};
	const char *names[2] = {name0, name1};
	sub_t sub[2];
	uint32_t cntw[2];
	int n, k;
	off[0] = 0; off[1] = strlen(name0); off[2] = off[1] + strlen(name1);
	if (off[2] >= sizeof(blob)) return -3;
	memcpy(blob, name0, off[1]); memcpy(blob + off[1], name1, off[2] - off[1]);
	for (k = 0; k < 2; ++k) { sub[k].s = sw[2 * k]; sub[k].del = 0; sub[k].e = sw[2 * k + 1]; }
	cntw[0] = c0; cntw[1] = c1;
	if (start == UINT32_MAX) n = snprintf(g_ref, REF_CAP, "x\tutg%.6dc\t%d\t%d\n", id1, len, n_reads);
	else if (have_sub)
		n = snprintf(g_ref, REF_CAP, "x\tutg%.6dl\t%d\t%d\t%d\t%d\t%s:%d-%d\t%c\t%s:%d-%d\t%c\n", id1, len, n_reads, cntw[1], cntw[0],
		             names[start >> 1], sub[start >> 1].s + 1, sub[start >> 1].e, "+-"[start & 1], names[end >> 1], sub[end >> 1].s + 1, sub[end >> 1].e, "+-"[end & 1]);
	else
		n = snprintf(g_ref, REF_CAP, "x\tutg%.6dl\t%d\t%d\t%d\t%d\t%s\t%c\t%s\t%c\n", id1, len, n_reads, cntw[1], cntw[0], names[start >> 1], "+-"[start & 1], names[end >> 1], "+-"[end & 1]);
	tc_ug_x(&cnt, id1, len, n_reads, start, end, c0, c1, &nm, have_sub ? sw : 0);
	if (cnt.n + 1 > cap) return -3;
	tc_ug_x(&st, id1, len, n_reads, start, end, c0, c1, &nm, have_sub ? sw : 0);
	return verdict(&cnt, &st, out, cap, g_ref, n);
}

/* the whole GFA of hand-made unitigs through tc_line_ug, record by record: its length; the bytes too when out is given and cap holds them; *n_nl = '\n' bytes the
 * routine reported.  -1: the passes disagree */
long long tu_dump(const tc_ug_t *g, uint64_t n_rec, const char *blob, const uint64_t *off, const uint32_t *sub, char *out, size_t cap, uint64_t *n_nl)
{
	const tc_names_t nm = {blob, off};
	uint64_t r, total = 0, nl = 0;
	for (r = 0; r < n_rec; ++r) {
		tc_emit_t cnt = {0, 0};
		nl += tc_line_ug(&cnt, g, r, &nm, sub);
		if (out && total + cnt.n <= cap) {
			tc_emit_t st = {out + total, 0};
			tc_line_ug(&st, g, r, &nm, sub);
			if (st.n != cnt.n) return -1;
		}
		total += cnt.n;
	}
	if (n_nl) *n_nl = nl;
	return (long long)total;
}

int tu_fixed(int which) { return which == 0 ? TC_FIXED_UG_S : which == 1 ? TC_FIXED_UG_A : which == 2 ? TC_FIXED_UG_L : which == 3 ? TC_FIXED_UG_X : TC_FIXED_UG; }
size_t tu_sizeof_ug(void) { return sizeof(tc_ug_t); }
