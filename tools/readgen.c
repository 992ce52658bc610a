/* readgen -- TEST/BENCH TOOL: a reads file (FASTA or FASTQ) that matches a PAF: every read name the PAF mentions, in order of first appearance, with
 * the first length the PAF gives for it (what the dictionary keeps, sdict.c:27-45) and random bases.  For `miniasm -f reads paf`.
 *
 * Usage: readgen [-q] [-w N] [-s seed] [-x frac] [-e N] [-o out] in.paf
 *     -q       FASTQ (four lines a record, constant quality); default FASTA
 *     -w N     FASTA: wrap the sequence at N bases a line (default 0: one line)
 *     -s seed  seed of the generator (default 1)
 *     -x frac  leave this fraction of the reads out (their positions in the unitigs stay N)
 *     -e N     N extra reads the PAF never names, spread through the file
 * Bases come from xorshift64* words, 32 bases a word, so tens of GB are a matter of the disk. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <unistd.h>

static uint64_t g_x = 88172645463325252ull;
static inline uint64_t rnd(void) { g_x ^= g_x >> 12; g_x ^= g_x << 25; g_x ^= g_x >> 27; return g_x * 2685821657736338717ull; }

/* names seen so far: open addressing over FNV-1a, names kept in one block */
typedef struct { uint64_t h; size_t off; uint32_t len, used; } slot_t;
static slot_t *g_tab; static size_t g_cap, g_n; static char *g_names; static size_t g_nb, g_nm;
static uint64_t fnv(const char *s, size_t l) { uint64_t h = 0xcbf29ce484222325ull; size_t i; for (i = 0; i < l; ++i) h = (h ^ (unsigned char)s[i]) * 0x100000001b3ull; return h; }
static int seen_put(const char *s, size_t l)
{
	uint64_t h = fnv(s, l);
	size_t i;
	if ((g_n + 1) * 2 > g_cap) { /* grow */
		size_t oc = g_cap, k; slot_t *ot = g_tab;
		g_cap = g_cap ? g_cap * 2 : 1 << 16; g_tab = (slot_t*)calloc(g_cap, sizeof(slot_t));
		for (k = 0; k < oc; ++k) if (ot[k].used) { for (i = ot[k].h & (g_cap - 1); g_tab[i].used; i = (i + 1) & (g_cap - 1)); g_tab[i] = ot[k]; }
		free(ot);
	}
	for (i = h & (g_cap - 1); g_tab[i].used; i = (i + 1) & (g_cap - 1)) if (g_tab[i].h == h && g_tab[i].len == l && memcmp(g_names + g_tab[i].off, s, l) == 0) return 0;
	if (g_nb + l > g_nm) { g_nm = (g_nb + l) * 2 + 4096; g_names = (char*)realloc(g_names, g_nm); }
	memcpy(g_names + g_nb, s, l);
	g_tab[i].h = h; g_tab[i].off = g_nb; g_tab[i].len = (uint32_t)l; g_tab[i].used = 1;
	g_nb += l; ++g_n;
	return 1;
}

static char *g_line; static size_t g_lm;
static void emit(FILE *out, const char *name, size_t nl, uint64_t len, int fq, uint64_t wrap)
{
	uint64_t i, need = len + (wrap ? len / wrap + 2 : 2), n = 0, col = 0;
	if (need > g_lm) { g_lm = need * 2; g_line = (char*)realloc(g_line, g_lm); }
	fputc(fq ? '@' : '>', out); fwrite(name, 1, nl, out); fputc('\n', out);
	for (i = 0; i < len;) {
		uint64_t w = rnd();
		int k;
		for (k = 0; k < 32 && i < len; ++k, ++i, w >>= 2) {
			g_line[n++] = "ACGT"[w & 3];
			if (wrap && !fq && ++col == wrap && i + 1 < len) g_line[n++] = '\n', col = 0;
		}
	}
	g_line[n++] = '\n';
	fwrite(g_line, 1, n, out);
	if (fq) { fputs("+\n", out); memset(g_line, 'I', len); g_line[len] = '\n'; fwrite(g_line, 1, len + 1, out); }
}

int main(int argc, char *argv[])
{
	int c, fq = 0, f;
	uint64_t wrap = 0, n_extra = 0, n_done = 0, every = 0;
	double drop = 0;
	const char *ofn = 0;
	FILE *in, *out;
	char *ln = 0; size_t lm = 0; ssize_t l;
	while ((c = getopt(argc, argv, "qw:s:x:e:o:")) >= 0) {
		if (c == 'q') fq = 1; else if (c == 'w') wrap = strtoull(optarg, 0, 10); else if (c == 's') g_x ^= strtoull(optarg, 0, 10) * 0x9e3779b97f4a7c15ull;
		else if (c == 'x') drop = atof(optarg); else if (c == 'e') n_extra = strtoull(optarg, 0, 10); else if (c == 'o') ofn = optarg;
	}
	if (optind >= argc) { fprintf(stderr, "Usage: readgen [-q] [-w N] [-s seed] [-x frac] [-e N] [-o out] in.paf\n"); return 1; }
	if ((in = fopen(argv[optind], "r")) == 0) { perror(argv[optind]); return 1; }
	out = ofn ? fopen(ofn, "w") : stdout;
	if (out == 0) { perror(ofn); return 1; }
	setvbuf(out, 0, _IOFBF, 1 << 22);
	if (g_x == 0) g_x = 1;
	every = n_extra ? 16 : 0;
	while ((l = getline(&ln, &lm, in)) > 0) {
		char *col[8], *p = ln;
		for (f = 0; f < 7; ++f) { col[f] = p; p = strchr(p, '\t'); if (p == 0) break; *p++ = 0; }
		if (f < 7) continue;
		for (f = 0; f < 6; f += 5) { /* query name + length, target name + length */
			size_t nl = strlen(col[f]);
			if (!seen_put(col[f], nl)) continue;
			if (n_extra && n_done % every == 0) { char nm[64]; int k = snprintf(nm, sizeof(nm), "readgen_extra_%llu", (unsigned long long)n_extra); emit(out, nm, (size_t)k, 500 + rnd() % 4000, fq, wrap); --n_extra; }
			++n_done;
			if (drop > 0 && (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) < drop) continue;
			emit(out, col[f], nl, strtoull(col[f + 1], 0, 10), fq, wrap);
		}
	}
	while (n_extra) { char nm[64]; int k = snprintf(nm, sizeof(nm), "readgen_extra_%llu", (unsigned long long)n_extra); emit(out, nm, (size_t)k, 500 + rnd() % 4000, fq, wrap); --n_extra; }
	fprintf(stderr, "[readgen] %llu reads named by the PAF\n", (unsigned long long)g_n);
	if (out != stdout) fclose(out);
	return 0;
}
