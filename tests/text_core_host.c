/* text_core.h compiled for the host: lets the CPU tests check the dump lines -- the length pass and the write pass of the same
 * routine -- against Python's % formatting and the reference binary, without a GPU (tests/test_text_core_cpu.py). */
#include <stdint.h>
#include <stddef.h>
#include "text_core.h"

/* line r of a dump: its length; the bytes too when out is given and cap holds them.  -1: the two passes disagree (they cannot) */
long tc_host_line(int kind, uint64_t r, const uint32_t *rec, const char *blob, const uint64_t *off, const uint32_t *sub, const uint8_t *del, char *out, size_t cap)
{
	tc_names_t nm = {blob, off};
	tc_emit_t cnt = {0, 0};
	tc_line(&cnt, kind, r, rec, &nm, sub, del);
	if (out && cnt.n <= cap) {
		tc_emit_t st = {out, 0};
		tc_line(&st, kind, r, rec, &nm, sub, del);
		if (st.n != cnt.n) return -1;
	}
	return (long)cnt.n;
}

/* the whole dump of n records: its length; the bytes too when out is given and cap holds them */
long long tc_host_dump(int kind, uint64_t n, const uint32_t *rec, const char *blob, const uint64_t *off, const uint32_t *sub, const uint8_t *del, char *out, size_t cap)
{
	tc_names_t nm = {blob, off};
	uint64_t r, total = 0;
	for (r = 0; r < n; ++r) {
		tc_emit_t cnt = {0, 0};
		tc_line(&cnt, kind, r, rec, &nm, sub, del);
		if (out && total + cnt.n <= cap) {
			tc_emit_t st = {out + total, 0};
			tc_line(&st, kind, r, rec, &nm, sub, del);
			if (st.n != cnt.n) return -1;
		}
		total += cnt.n;
	}
	return (long long)total;
}

/* every v < 100000: the five digits of tc_dig5 against the quotients; every power of ten and its neighbours: tc_ndig.  Returns the number of mismatches */
long tc_host_digit_check(void)
{
	long bad = 0;
	uint32_t v, d[5], p;
	int k;
	for (v = 0; v < 100000u; ++v) {
		tc_dig5(v, d);
		if (d[0] != v / 10000u || d[1] != v / 1000u % 10u || d[2] != v / 100u % 10u || d[3] != v / 10u % 10u || d[4] != v % 10u) ++bad;
	}
	for (p = 1, k = 1; k <= 10; ++k) {
		if (tc_ndig(p) != (uint32_t)k || tc_ndig(p - 1) != (uint32_t)(k > 1 ? k - 1 : 1)) ++bad;
		if (k < 10) p *= 10u;
	}
	if (tc_ndig(0xffffffffu) != 10) ++bad;
	return bad;
}

int tc_host_fixed(int kind) { return kind == TC_KIND_PAF ? TC_FIXED_PAF : kind == TC_KIND_SG ? TC_FIXED_SG : TC_FIXED_BED; }
