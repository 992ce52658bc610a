/* asm.c -- hits -> string graph bridge (GPU), unitig construction (GPU) and the GFA / string-graph writers (host).
 * Reference: asm.c:9-39 (ma_sg_gen), :41-55 (ma_sg_print), :64-116 (ma_ug_destroy, ma_ug_print),
 * :121-210 (ma_ug_gen), :216-290 (ma_ug_seq).
 * The output line formats are the contract with downstream tools and are reproduced byte for byte.
 */
#include <stdio.h>
#include <stdlib.h>
#include <pthread.h>
#include <string.h>
#include "ma_host.h"

#define GPU(call) do { if ((call) != 0) ma_gpu_fail(__func__); } while (0)

asg_arc_t *ma_asg_arc_pushp(asg_t *g);

asg_t *ma_sg_gen(const ma_opt_t *opt, const sdict_t *d, const ma_sub_t *sub, size_t n_hits, const ma_hit_t *hit)
{
	mahip_ctx_t *c = ma_gpu();
	asg_t *g = asg_init();
	uint32_t i, n_arc = 0, R = d->n_seq;
	uint8_t *del = (uint8_t*)malloc(R ? R : 1);
	uint32_t *len = 0;
	for (i = 0; i < R; ++i) del[i] = d->seq[i].del;
	if (!sub) {
		len = (uint32_t*)malloc((R ? R : 1) * 4);
		for (i = 0; i < R; ++i) len[i] = d->seq[i].len;
	}
	GPU(mahip_set_shard(c, 0, 0xffffffffu));
	GPU(mahip_hits_upload(c, hit, n_hits, R));
	GPU(mahip_hits_index(c));
	if (sub) GPU(mahip_sub_upload(c, 0, sub, R));
	GPU(mahip_sg_gen(c, opt, sub != 0, len, del, &n_arc));
	GPU(mahip_asg_download(c, g));
	free(del); free(len);
	fprintf(MA_LOG, "[M::%s] read %d arcs\n", __func__, g->n_arc);
	return g;
}

/* ---- buffered text output: the writers below produce tens of thousands of short lines; formatting them with
 * fprintf costs more than every GPU pass together, so lines are assembled in a buffer with hand-rolled integer
 * formatting and written once.  Byte-for-byte the text the reference's fprintf calls produce. */
typedef struct { char *s; size_t n, m; FILE *fp; } obuf_t;

static inline void ob_need(obuf_t *o, size_t k)
{
	if (o->n + k > o->m) {
		o->m = (o->n + k) * 2 + 4096;
		o->s = (char*)realloc(o->s, o->m);
	}
}
static inline void ob_chr(obuf_t *o, char c) { ob_need(o, 1); o->s[o->n++] = c; }
static inline void ob_mem(obuf_t *o, const char *p, size_t l) { ob_need(o, l); memcpy(o->s + o->n, p, l); o->n += l; }
static inline void ob_str(obuf_t *o, const char *p) { ob_mem(o, p, strlen(p)); }
static inline void ob_int(obuf_t *o, int64_t x) /* %d */
{
	char t[24]; int k = 0; uint64_t u = x < 0 ? (uint64_t)(-x) : (uint64_t)x;
	do { t[k++] = (char)('0' + u % 10); u /= 10; } while (u);
	ob_need(o, (size_t)k + 1);
	if (x < 0) o->s[o->n++] = '-';
	while (k) o->s[o->n++] = t[--k];
}
static inline void ob_int6(obuf_t *o, uint32_t x) /* %.6d of a non-negative value */
{
	char t[24]; int k = 0;
	do { t[k++] = (char)('0' + x % 10); x /= 10; } while (x);
	while (k < 6) t[k++] = '0';
	ob_need(o, (size_t)k);
	while (k) o->s[o->n++] = t[--k];
}
static inline void ob_flush(obuf_t *o) { if (o->n) fwrite(o->s, 1, o->n, o->fp); free(o->s); o->s = 0; o->n = o->m = 0; }
/* "name:s+1-e" (or just the name without sub) */
static inline void ob_read(obuf_t *o, const sdict_t *d, const ma_sub_t *sub, uint32_t x)
{
	ob_str(o, d->seq[x].name);
	if (sub) { ob_chr(o, ':'); ob_int(o, (int)sub[x].s + 1); ob_chr(o, '-'); ob_int(o, (int)sub[x].e); }
}

void ma_sg_print(const asg_t *g, const sdict_t *d, const ma_sub_t *sub, FILE *fp) /* asm.c:41-55 */
{
	uint32_t i;
	obuf_t o = {0, 0, 0, fp};
	for (i = 0; i < g->n_arc; ++i) { /* "L\t%s:%d-%d\t%c\t%s:%d-%d\t%c\t%d:\tL1:i:%d\n" */
		const asg_arc_t *p = &g->arc[i];
		ob_mem(&o, "L\t", 2); ob_read(&o, d, sub, (uint32_t)(p->ul >> 33)); ob_chr(&o, '\t'); ob_chr(&o, "+-"[p->ul >> 32 & 1]); ob_chr(&o, '\t');
		ob_read(&o, d, sub, p->v >> 1); ob_chr(&o, '\t'); ob_chr(&o, "+-"[p->v & 1]); ob_chr(&o, '\t');
		ob_int(&o, (int)p->ol); ob_mem(&o, ":\tL1:i:", 7); ob_int(&o, (int)(uint32_t)p->ul); ob_chr(&o, '\n');
	}
	ob_flush(&o);
}

/* ---------------------------------------------------------------------------------------------- unitigs */

void ma_ug_destroy(ma_ug_t *ug)
{
	size_t i;
	if (ug == 0) return;
	for (i = 0; i < ug->u.n; ++i) { free(ug->u.a[i].a); free(ug->u.a[i].s); }
	free(ug->u.a);
	asg_destroy(ug->g);
	free(ug);
}

/* asm.c:121-210.  The unitigs are computed on the device (csrc/ug.hip: links, list ranking by pointer jumping, orientation and
 * numbering by the discovery vertex, segmented gather of the members); the host only unpacks the arrays into the reference's
 * ma_ug_t and finishes the (small) unitig graph: asg_cleanup = the reference's sort order + index (asm.c:208). */
ma_ug_t *ma_ug_from_device(mahip_ctx_t *c)
{
	uint32_t U = 0, M = 0, NA = 0;
	GPU(mahip_ug_gen(c, &U, &M, &NA));
	return ma_ug_unpack(c, U, M, NA);
}

/* the second half of ma_ug_from_device: the unitigs mahip_ug_gen left in the context (its three counts), unpacked */
ma_ug_t *ma_ug_unpack(mahip_ctx_t *c, uint32_t U, uint32_t M, uint32_t NA)
{
	ma_ug_t *ug = (ma_ug_t*)calloc(1, sizeof(ma_ug_t));
	uint32_t *u_n, *u_len, *u_start, *u_end, *u_off, k;
	uint64_t *mem;
	ug->g = asg_init();
	u_n = (uint32_t*)malloc(((size_t)U + 1) * 4 * 5);
	u_len = u_n + U; u_start = u_len + U; u_end = u_start + U; u_off = u_end + U;
	mem = (uint64_t*)malloc(((size_t)M + 1) * 8);
	ug->g->arc = (asg_arc_t*)malloc(((size_t)NA + 1) * sizeof(asg_arc_t));
	ug->g->m_arc = NA + 1; ug->g->n_arc = NA;
	GPU(mahip_ug_download(c, u_n, u_len, u_start, u_end, u_off, mem, ug->g->arc));
	ug->u.n = ug->u.m = U;
	ug->u.a = (ma_utg_t*)calloc(U ? U : 1, sizeof(ma_utg_t));
	for (k = 0; k < U; ++k) {
		ma_utg_t *p = &ug->u.a[k];
		uint32_t m = u_n[k];
		p->len = u_len[k]; p->circ = u_start[k] == UINT32_MAX;
		p->start = u_start[k]; p->end = u_end[k];
		p->n = m;
		if (m) { --m; m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16; ++m; }
		p->m = m;
		p->a = (uint64_t*)malloc(8 * (size_t)(p->m ? p->m : 1));
		memcpy(p->a, mem + u_off[k], (size_t)p->n * 8);
		asg_seq_set(ug->g, (int)k, (int)p->len, 0);
	}
	free(u_n); free(mem);
	asg_cleanup(ug->g);
	return ug;
}

/* the unitig arcs alone, in the reference's order (what asg_cleanup makes of them above: no arc is deleted, so it is the sort): all the device text writer needs
 * on the host.  free() the result */
asg_arc_t *ma_ug_links_from_device(mahip_ctx_t *c, uint32_t NA)
{
	asg_arc_t *a = (asg_arc_t*)malloc(((size_t)NA + 1) * sizeof(asg_arc_t));
	GPU(mahip_ug_download(c, 0, 0, 0, 0, 0, 0, a));
	ma_refsort_arcs(a, a + NA);
	return a;
}

ma_ug_t *ma_ug_gen(asg_t *g) /* per-symbol form: the caller's host graph goes up first */
{
	mahip_ctx_t *c = ma_gpu();
	if (!g->is_srt || g->idx == 0) asg_cleanup(g);
	GPU(mahip_asg_upload(c, g));
	return ma_ug_from_device(c);
}

static inline void ob_utg(obuf_t *o, uint32_t id1, int circ) { ob_mem(o, "utg", 3); ob_int6(o, id1); ob_chr(o, "lc"[circ]); }

/* The three blocks of a unitig GFA (asm.c:77-116).  Formatting is bound by cache misses on names and intervals of reads
 * scattered over the dictionary, so big outputs are formatted by several threads, each into its own buffer over a
 * contiguous range of unitigs / links, and written in order: the text is the sequential one byte for byte. */
/* a segment = reads [j0, j1) of unitig u, l0 = offset of read j0 on the unitig; the segment with j0 == 0 also carries the
 * S line (and the circularising L lines): long unitigs are cut into several segments so that they can be formatted in parallel */
typedef struct { uint32_t u, j0, j1, l0; } fmt_seg_t;

static void fmt_units(obuf_t *o, const ma_ug_t *ug, const sdict_t *d, const ma_sub_t *sub, const fmt_seg_t *seg, size_t lo, size_t hi)
{
	size_t k;
	uint32_t j, l;
	for (k = lo; k < hi; ++k) {
		const uint32_t i = seg[k].u;
		const ma_utg_t *p = &ug->u.a[i];
		if (seg[k].j0 == 0) { /* S line, circularising L lines */
			ob_mem(o, "S\t", 2); ob_utg(o, i + 1, p->circ); ob_chr(o, '\t'); ob_str(o, p->s ? p->s : "*"); ob_mem(o, "\tLN:i:", 6); ob_int(o, (int)p->len); ob_chr(o, '\n');
			if (p->circ) {
				for (j = 0; j < 2; ++j) { /* "L\t%s\t+\t%s\t+\t0M\n" and the '-' twin */
					char c = "+-"[j];
					ob_mem(o, "L\t", 2); ob_utg(o, i + 1, p->circ); ob_chr(o, '\t'); ob_chr(o, c); ob_chr(o, '\t');
					ob_utg(o, i + 1, p->circ); ob_chr(o, '\t'); ob_chr(o, c); ob_mem(o, "\t0M\n", 4);
				}
			}
		}
		for (j = seg[k].j0, l = seg[k].l0; j < seg[k].j1; l += (uint32_t)p->a[j++]) { /* "a\t%s\t%d\t%s:%d-%d\t%c\t%d\n" */
			if (j + 4 < p->n) __builtin_prefetch(&d->seq[p->a[j + 4] >> 33]);
			if (j + 2 < p->n) __builtin_prefetch(d->seq[p->a[j + 2] >> 33].name);
			ob_mem(o, "a\t", 2); ob_utg(o, i + 1, p->circ); ob_chr(o, '\t'); ob_int(o, (int)l); ob_chr(o, '\t');
			ob_read(o, d, sub, (uint32_t)(p->a[j] >> 33)); ob_chr(o, '\t'); ob_chr(o, "+-"[p->a[j] >> 32 & 1]); ob_chr(o, '\t');
			ob_int(o, (int)(uint32_t)p->a[j]); ob_chr(o, '\n');
		}
	}
}

static void fmt_links(obuf_t *o, const ma_ug_t *ug, uint32_t lo, uint32_t hi)
{
	uint32_t i;
	for (i = lo; i < hi; ++i) { /* "L\tutg%.6d%c\t%c\tutg%.6d%c\t%c\t%dM\tSD:i:%d\n" */
		const asg_arc_t *e = &ug->g->arc[i];
		uint32_t u = (uint32_t)(e->ul >> 32), v = e->v;
		ob_mem(o, "L\t", 2); ob_utg(o, (u >> 1) + 1, ug->u.a[u >> 1].circ); ob_chr(o, '\t'); ob_chr(o, "+-"[u & 1]); ob_chr(o, '\t');
		ob_utg(o, (v >> 1) + 1, ug->u.a[v >> 1].circ); ob_chr(o, '\t'); ob_chr(o, "+-"[v & 1]); ob_chr(o, '\t');
		ob_int(o, (int)e->ol); ob_mem(o, "M\tSD:i:", 7); ob_int(o, (int)asg_arc_len(*e)); ob_chr(o, '\n');
	}
}

static void fmt_summary(obuf_t *o, const ma_ug_t *ug, const sdict_t *d, const ma_sub_t *sub, uint32_t lo, uint32_t hi)
{
	uint32_t i;
	for (i = lo; i < hi; ++i) { /* x lines: unitig summary */
		const ma_utg_t *u = &ug->u.a[i];
		if (u->start == UINT32_MAX) { /* "x\tutg%.6dc\t%d\t%d\n" */
			ob_mem(o, "x\t", 2); ob_utg(o, i + 1, 1); ob_chr(o, '\t'); ob_int(o, (int)u->len); ob_chr(o, '\t'); ob_int(o, (int)u->n); ob_chr(o, '\n');
		} else { /* "x\tutg%.6dl\t%d\t%d\t%d\t%d\t%s:%d-%d\t%c\t%s:%d-%d\t%c\n" */
			uint32_t c0 = asg_arc_n(ug->g, i << 1 | 0), c1 = asg_arc_n(ug->g, i << 1 | 1);
			ob_mem(o, "x\t", 2); ob_utg(o, i + 1, 0); ob_chr(o, '\t'); ob_int(o, (int)u->len); ob_chr(o, '\t'); ob_int(o, (int)u->n); ob_chr(o, '\t');
			ob_int(o, (int)c1); ob_chr(o, '\t'); ob_int(o, (int)c0); ob_chr(o, '\t');
			ob_read(o, d, sub, u->start >> 1); ob_chr(o, '\t'); ob_chr(o, "+-"[u->start & 1]); ob_chr(o, '\t');
			ob_read(o, d, sub, u->end >> 1); ob_chr(o, '\t'); ob_chr(o, "+-"[u->end & 1]); ob_chr(o, '\n');
		}
	}
}

typedef struct { const ma_ug_t *ug; const sdict_t *d; const ma_sub_t *sub; const fmt_seg_t *seg; size_t s_lo, s_hi; uint32_t u_lo, u_hi, l_lo, l_hi; obuf_t units, links, summary; } fmt_job_t;

static void *fmt_worker(void *arg)
{
	fmt_job_t *j = (fmt_job_t*)arg;
	{ /* room for the whole share up front (an `a` line is about 40 bytes, an `L` line 45, an `x` line 70): a buffer that grows by doubling copies its text again and again and touches twice the pages */
		size_t k, reads = 0;
		for (k = j->s_lo; k < j->s_hi; ++k) reads += (size_t)(j->seg[k].j1 - j->seg[k].j0) + 2;
		ob_need(&j->units, reads * 52 + 4096);
		ob_need(&j->links, (size_t)(j->l_hi - j->l_lo) * 56 + 4096);
		ob_need(&j->summary, (size_t)(j->u_hi - j->u_lo) * 96 + 4096);
	}
	fmt_units(&j->units, j->ug, j->d, j->sub, j->seg, j->s_lo, j->s_hi);
	fmt_links(&j->links, j->ug, j->l_lo, j->l_hi);
	fmt_summary(&j->summary, j->ug, j->d, j->sub, j->u_lo, j->u_hi);
	return 0;
}

#define FMT_MAX_THREADS 16
#define FMT_SEG_READS 2048u
extern double g_fmt_laps[2]; /* pipeline.c */
typedef struct { fmt_job_t *job; int T, t; char *dst; } fmt_copy_t;
static void *fmt_copy_worker(void *arg) /* thread t copies ITS three pieces to their places: the pages of a fresh block are first touched by sixteen threads, not one */
{
	fmt_copy_t *q = (fmt_copy_t*)arg;
	size_t off_u = 0, off_l = 0, off_s = 0;
	int t;
	for (t = 0; t < q->T; ++t) off_l += q->job[t].units.n;
	off_s = off_l;
	for (t = 0; t < q->T; ++t) off_s += q->job[t].links.n;
	for (t = 0; t < q->t; ++t) { off_u += q->job[t].units.n; off_l += q->job[t].links.n; off_s += q->job[t].summary.n; }
	memcpy(q->dst + off_u, q->job[q->t].units.s, q->job[q->t].units.n);
	memcpy(q->dst + off_l, q->job[q->t].links.s, q->job[q->t].links.n);
	memcpy(q->dst + off_s, q->job[q->t].summary.s, q->job[q->t].summary.n);
	return 0;
}
/* asm.c:77-116: the text goes to fp, or (fp == 0) into one malloc'ed block *buf of *len bytes */
static void ug_print_to(const ma_ug_t *ug, const sdict_t *d, const ma_sub_t *sub, FILE *fp, char **buf, size_t *len)
{
	const uint32_t nu = (uint32_t)ug->u.n, nl = ug->g->n_arc;
	uint64_t tot = 0, acc = 0;
	uint32_t i, j, l;
	size_t n_seg = 0, m_seg = (size_t)nu + 16, si;
	int T, t, k;
	fmt_seg_t *seg = (fmt_seg_t*)malloc(m_seg * sizeof(fmt_seg_t));
	const char *e_seg = getenv("MA_FMT_SEG"); /* reads per segment (tests shrink it to cut short unitigs too) */
	const uint32_t seg_reads = e_seg && atol(e_seg) > 0 ? (uint32_t)atol(e_seg) : FMT_SEG_READS;
	fmt_job_t job[FMT_MAX_THREADS];
	pthread_t th[FMT_MAX_THREADS];
	int started[FMT_MAX_THREADS];
	for (i = 0; i < nu; ++i) { /* segments in output order */
		const ma_utg_t *p = &ug->u.a[i];
		tot += p->n + 2;
		j = 0; l = 0;
		do {
			uint32_t j1 = p->n - j > seg_reads ? j + seg_reads : p->n, x;
			if (n_seg == m_seg) { m_seg <<= 1; seg = (fmt_seg_t*)realloc(seg, m_seg * sizeof(fmt_seg_t)); }
			seg[n_seg].u = i; seg[n_seg].j0 = j; seg[n_seg].j1 = j1; seg[n_seg].l0 = l; ++n_seg;
			for (x = j; x < j1; ++x) l += (uint32_t)p->a[x];
			j = j1;
		} while (j < p->n);
	}
	{
		const char *e = getenv("MA_FMT_GRAIN"); /* lines per thread at least: about 0.3 ms of formatting */
		long grain = e ? atol(e) : 6000;
		T = (int)(tot / (uint64_t)(grain > 0 ? grain : 1));
	}
	k = ma_ingest_threads();
	if (T > k) T = k;
	if (T > FMT_MAX_THREADS) T = FMT_MAX_THREADS;
	if (T < 1) T = 1;
	memset(job, 0, sizeof(job));
	for (t = 0, si = 0; t < T; ++t) { /* segment ranges of about equal read count; summary lines by unitig range, links by equal share */
		uint64_t want = tot * (uint64_t)(t + 1) / (uint64_t)T;
		job[t].ug = ug; job[t].d = d; job[t].sub = sub; job[t].seg = seg;
		job[t].s_lo = si;
		while (si < n_seg && (acc < want || t == T - 1)) { acc += (seg[si].j1 - seg[si].j0) + (seg[si].j0 == 0 ? 2 : 0); ++si; }
		job[t].s_hi = si;
		job[t].u_lo = (uint32_t)((uint64_t)nu * (uint64_t)t / (uint64_t)T);
		job[t].u_hi = (uint32_t)((uint64_t)nu * (uint64_t)(t + 1) / (uint64_t)T);
		job[t].l_lo = (uint32_t)((uint64_t)nl * (uint64_t)t / (uint64_t)T);
		job[t].l_hi = (uint32_t)((uint64_t)nl * (uint64_t)(t + 1) / (uint64_t)T);
	}
	const int timing = ma_timing_level() >= 1;
	const double t_begin = sys_realtime();
	double t_fmt;
	for (t = 1; t < T; ++t) {
		started[t] = pthread_create(&th[t], 0, fmt_worker, &job[t]) == 0;
		if (!started[t]) fmt_worker(&job[t]);
	}
	fmt_worker(&job[0]);
	for (t = 1; t < T; ++t) if (started[t]) pthread_join(th[t], 0);
	t_fmt = sys_realtime();
	if (fp) {
		for (t = 0; t < T; ++t) { job[t].units.fp = fp; ob_flush(&job[t].units); }
		for (t = 0; t < T; ++t) { job[t].links.fp = fp; ob_flush(&job[t].links); }
		for (t = 0; t < T; ++t) { job[t].summary.fp = fp; ob_flush(&job[t].summary); }
	} else { /* one block, every thread copies what it formatted */
		fmt_copy_t cp[FMT_MAX_THREADS];
		size_t total = 0;
		char *dst;
		for (t = 0; t < T; ++t) total += job[t].units.n + job[t].links.n + job[t].summary.n;
		dst = (char*)ma_big_alloc(total + 1);
		for (t = 0; t < T; ++t) { cp[t].job = job; cp[t].T = T; cp[t].t = t; cp[t].dst = dst; }
		for (t = 1; t < T; ++t) {
			started[t] = pthread_create(&th[t], 0, fmt_copy_worker, &cp[t]) == 0;
			if (!started[t]) fmt_copy_worker(&cp[t]);
		}
		fmt_copy_worker(&cp[0]);
		for (t = 1; t < T; ++t) if (started[t]) pthread_join(th[t], 0);
		for (t = 0; t < T; ++t) { free(job[t].units.s); free(job[t].links.s); free(job[t].summary.s); }
		dst[total] = 0;
		*buf = dst; *len = total;
	}
	free(seg);
	g_fmt_laps[0] = (t_fmt - t_begin) * 1e3; g_fmt_laps[1] = (sys_realtime() - t_fmt) * 1e3;
	if (timing) fprintf(stderr, "[T::ug_print] %d threads: format %.3f ms, %s %.3f ms\n", T, (t_fmt - t_begin) * 1e3, fp ? "write" : "copy into one block", (sys_realtime() - t_fmt) * 1e3);
}

void ma_ug_print(const ma_ug_t *ug, const sdict_t *d, const ma_sub_t *sub, FILE *fp) { ug_print_to(ug, d, sub, fp, 0, 0); }
/* the same text in one malloc'ed block (free() it): what a caller that wants the GFA in memory gets without a stream in between */
void ma_ug_print_mem(const ma_ug_t *ug, const sdict_t *d, const ma_sub_t *sub, char **buf, size_t *len) { ug_print_to(ug, d, sub, 0, buf, len); }

/* ---------------------------------------------------------------------------------------------- unitig sequences
 * reference asm.c:216-290 (ma_ug_seq): every read placed on a unitig contributes the first `len` bases of its kept
 * interval (forward) or the reverse complement of its last `len` bases (reverse).  FASTA/FASTQ, plain or gzip, read
 * with the record rules of the reference's reader (kseq.h:172-247): a record starts at a line beginning with '>' or
 * '@', the name ends at the first white space, sequence lines run until a line starting with '>', '@' or '+', a '+'
 * line is followed by as many quality characters as there are bases. */
#include <zlib.h>
#include <ctype.h>
#include <assert.h>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>

/* the bytes of the stream: fp, and in front of it (pre != 0) up to FQ_SEGS stretches of memory -- what the streamed device reader had taken from fp when it handed
 * over (below) */
#define FQ_SEGS 3
typedef struct { struct { const unsigned char *p; size_t len; } seg[FQ_SEGS]; int i; } fq_pre_t;
typedef struct { gzFile fp; unsigned char *buf; int beg, end, eof; fq_pre_t *pre; } fq_stream_t;
#define FQ_BUF (1 << 18)

/* the next FQ_BUF bytes (fewer: the end of the input), as gzread returns them.  Out of line and without the stream's address: fq_getc runs once per byte, and the
 * cursor of a stream whose address goes nowhere stays in registers */
static int __attribute__((noinline)) fq_fill(gzFile fp, unsigned char *buf, fq_pre_t *pre)
{
	int n = 0, got;
	while (pre && pre->i < FQ_SEGS && n < FQ_BUF) {
		const size_t k = pre->seg[pre->i].len < (size_t)(FQ_BUF - n) ? pre->seg[pre->i].len : (size_t)(FQ_BUF - n);
		if (k == 0) { ++pre->i; continue; }
		memcpy(buf + n, pre->seg[pre->i].p, k);
		pre->seg[pre->i].p += k; pre->seg[pre->i].len -= k;
		n += (int)k;
	}
	if (n == FQ_BUF) return n;
	got = gzread(fp, buf + n, FQ_BUF - n);
	return got > 0 ? n + got : n ? n : got;
}

static inline int fq_getc(fq_stream_t *f)
{
	if (f->beg >= f->end) {
		if (f->eof) return -1;
		f->beg = 0; f->end = fq_fill(f->fp, f->buf, f->pre);
		if (f->end < FQ_BUF) f->eof = 1;
		if (f->end <= 0) { f->end = 0; return -1; }
	}
	return f->buf[f->beg++];
}

typedef struct { char *s; size_t l, m; } fq_str_t;
static inline void fq_push(fq_str_t *t, int c)
{
	if (t->l + 2 > t->m) { t->m = t->m ? t->m << 1 : 256; t->s = (char*)realloc(t->s, t->m); }
	t->s[t->l++] = (char)c; t->s[t->l] = 0;
}
/* append the rest of the current line (without the line end, CR dropped like kseq.h:146 when the line is longer than 1) */
static int fq_line(fq_stream_t *f, fq_str_t *t)
{
	int c;
	size_t l0 = t->l;
	while ((c = fq_getc(f)) != -1 && c != '\n') fq_push(t, c);
	if (t->l - l0 > 1 && t->s[t->l - 1] == '\r') t->s[--t->l] = 0;
	return c;
}

/* next record: name and sequence (qualities are skipped); *last is the look-ahead marker; returns <0 at end (-2: quality string of another length than the sequence) */
static int fq_read(fq_stream_t *f, int *last, fq_str_t *name, fq_str_t *seq)
{
	int c;
	if (*last == 0) {
		while ((c = fq_getc(f)) != -1 && c != '>' && c != '@');
		if (c == -1) return -1;
		*last = c;
	}
	name->l = seq->l = 0;
	if (name->s) name->s[0] = 0;
	while ((c = fq_getc(f)) != -1 && !isspace(c)) fq_push(name, c); /* name up to the first white space */
	if (c == -1 && name->l == 0) return -1;
	if (c != '\n' && c != -1) while ((c = fq_getc(f)) != -1 && c != '\n'); /* comment */
	if (seq->s == 0) { seq->m = 256; seq->s = (char*)malloc(seq->m); }
	seq->s[0] = 0;
	while ((c = fq_getc(f)) != -1 && c != '>' && c != '+' && c != '@') {
		if (c == '\n') continue; /* empty line */
		fq_push(seq, c);
		fq_line(f, seq);
	}
	if (c == '>' || c == '@') *last = c; else *last = 0;
	if (c == '+') { /* FASTQ: skip the '+' line, then whole quality LINES until they hold as many characters as there are bases (kseq.h:226-230) */
		size_t ql = 0;
		int tail = 0; /* last quality character kept so far */
		while ((c = fq_getc(f)) != -1 && c != '\n');
		if (c == -1) return -2; /* no quality string */
		do {
			if ((c = fq_getc(f)) == -1) break; /* nothing left to read */
			for (; c != -1 && c != '\n'; c = fq_getc(f)) ++ql, tail = c;
			if (ql > 1 && tail == '\r') --ql, tail = 0; /* kseq.h:146 */
		} while (ql < seq->l);
		*last = 0;
		if (ql != seq->l) return -2; /* the reference's loop (asm.c:262) stops reading the file here */
	}
	return (int)seq->l;
}

typedef struct { uint32_t utg:31, ori:1, start, len; } utg_place_t;

/* the reads that sit on a unitig as the device readers want them (include/mahip.h: mahip_useq_want_t): name, where the bases go, strand, kept interval; free() both */
static void ug_seq_wanted(const sdict_t *d, const ma_sub_t *sub, const utg_place_t *pl, const uint64_t *uoff, mahip_useq_want_t **want_, char **names_, size_t *n_want_, size_t *name_bytes_)
{
	mahip_useq_want_t *want;
	char *names;
	size_t n_want = 0, name_bytes = 0;
	uint32_t i;
	for (i = 0; i < d->n_seq; ++i) if (pl[i].len) ++n_want, name_bytes += strlen(d->seq[i].name);
	want = (mahip_useq_want_t*)malloc((n_want ? n_want : 1) * sizeof(mahip_useq_want_t));
	names = (char*)malloc(name_bytes ? name_bytes : 1);
	n_want = name_bytes = 0;
	for (i = 0; i < d->n_seq; ++i) {
		const utg_place_t *t = &pl[i];
		mahip_useq_want_t *w = &want[n_want];
		const size_t l = strlen(d->seq[i].name);
		if (t->len == 0 || l == 0) continue; /* (no record has an empty name that matches) */
		memcpy(names + name_bytes, d->seq[i].name, l);
		w->dst_off = uoff[t->utg] + t->start; w->name_off = name_bytes; w->name_len = (uint32_t)l;
		w->len = t->len; w->rev = t->ori; w->whole = sub == 0;
		w->s = sub ? sub[i].s : 0; w->e = sub ? sub[i].e : 0;
		++n_want; name_bytes += l;
	}
	*want_ = want; *names_ = names; *n_want_ = n_want; *name_bytes_ = name_bytes;
}

/* The reads file on the device (csrc/useq.hip): a plain file goes to HBM as it is; the device checks that it is in the regular form (include/mahip.h), looks
 * the names of the reads that sit on a unitig up among its records and copies their bases into the arena.  Returns 1 when the arena is filled, 0 with
 * ui->reason when the host reader has to run (the arena is untouched then), -1 on an error.  pl == 0: the wanted reads are the table of the placement plan the
 * context holds (mahip_useq_plan), nothing is gathered or uploaded here. */
enum { LAP_LOAD, LAP_INDEX, LAP_LOOKUP, LAP_PLACE, LAP_DOWNLOAD, N_LAPS };
static int ug_seq_device(mahip_ctx_t *c, const sdict_t *d, const ma_sub_t *sub, const char *fn, const utg_place_t *pl, const uint64_t *uoff, mahip_useq_info_t *ui, double *laps)
{
	const char *e = getenv("MA_FASTX_HOST");
	struct stat st;
	unsigned char magic[2] = {0, 0};
	mahip_fastx_info_t fi;
	mahip_useq_want_t *want = 0;
	char *names = 0;
	size_t n_want = 0, name_bytes = 0;
	double t0, pl_laps[2];
	int fd, rc;
	if (e && atoi(e) != 0) { ui->reason = MAHIP_FASTX_FORCED; return 0; }
	ui->reason = MAHIP_FASTX_NOT_PLAIN;
	if (fn == 0 || strcmp(fn, "-") == 0) return 0;
	if ((fd = open(fn, O_RDONLY)) < 0) return 0; /* the host reader reports it */
	if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0 || pread(fd, magic, 2, 0) < 1) { close(fd); return 0; }
	t0 = sys_realtime();
	mahip_mem_trim(c, 0); /* what the passes before left idle in the pool: the text may need it */
	if (magic[0] == 0x1f && magic[1] == 0x8b) { /* compressed: bgzip's blocks are inflated on the device into the same text buffer (include/mahip.h), plain gzip too under MA_GZIP_DEVICE=1; anything else is NOT_PLAIN, as ever */
		mahip_bgzf_info_t bi;
		if (!ma_bgzf_enabled()) {
			memset(&bi, 0, sizeof(bi));
			bi.reader = MAHIP_BGZF_HOST; bi.reason = MAHIP_BGZF_FORCED; bi.first_bad_member = -1; bi.comp_bytes = (uint64_t)st.st_size;
			mahip_bgzf_note(c, &bi);
			close(fd);
			return 0;
		}
		rc = mahip_bgzf_load_fd(c, fd, (size_t)st.st_size, MAHIP_BGZF_FASTX, &bi);
		if (rc != 0) { close(fd); mahip_fastx_release(c); return -1; }
		if (bi.reason == MAHIP_BGZF_NOT_BGZF && ma_gzip_device_enabled()) { /* plain gzip, one member or several: the chunked inflater (MA_GZIP_DEVICE=1); any refusal is NOT_PLAIN */
			mahip_gzip_info_t gi;
			rc = mahip_gzip_load_fd_members(c, fd, (size_t)st.st_size, MAHIP_BGZF_FASTX, 0, &gi);
			close(fd);
			if (rc != 0) { mahip_fastx_release(c); return -1; }
			if (gi.reason != MAHIP_GZIP_OK) return 0;
		} else {
			close(fd);
			if (bi.reason != MAHIP_BGZF_OK) return 0;
		}
	} else {
		rc = mahip_fastx_load_fd(c, fd, (size_t)st.st_size);
		close(fd);
		if (rc < 0) { mahip_fastx_release(c); return -1; } /* a read error, a HIP error */
		if (rc > 0) { ui->reason = MAHIP_FASTX_NOMEM; mahip_fastx_release(c); return 0; } /* no room for the text */
	}
	laps[LAP_LOAD] = (sys_realtime() - t0) * 1e3; t0 = sys_realtime();
	if (mahip_fastx_index(c, &fi) != 0) { mahip_fastx_release(c); return -1; }
	laps[LAP_INDEX] = (sys_realtime() - t0) * 1e3;
	ui->format = fi.format; ui->n_records = fi.n_records;
	if (!fi.regular) { ui->reason = fi.reason; mahip_fastx_release(c); return 0; }
	if (pl) {
		ug_seq_wanted(d, sub, pl, uoff, &want, &names, &n_want, &name_bytes);
		rc = mahip_useq_place_text(c, want, n_want, names, name_bytes, &ui->n_matched, &ui->n_dup, &ui->n_short, pl_laps);
		free(want); free(names);
	} else rc = mahip_useq_place_text_planned(c, &ui->n_matched, &ui->n_dup, &ui->n_short, pl_laps);
	laps[LAP_LOOKUP] = pl_laps[0]; laps[LAP_PLACE] = pl_laps[1];
	if (mahip_fastx_release(c) != 0 || rc != 0) return -1;
	if (ui->n_short) { ui->reason = MAHIP_FASTX_SHORT_READ; return 0; }
	ui->reason = MAHIP_FASTX_OK;
	return 1;
}

/* MA_FASTX_STREAM: 0 or unset = off; 1 = the streamed device reader takes what the whole-file reader cannot (NOT_PLAIN: gzip, stdin, a FIFO, a bgzip file that is
 * refused or host-forced; NOMEM); 2 = it takes every reads file (tests and tools/useq_stream_time.py reach it with any text).  The default stays off: DESIGN 7 */
int ma_fastx_stream_mode(void)
{
	const char *s = getenv("MA_FASTX_STREAM");
	const int v = s && *s ? atoi(s) : 0;
	return v == 1 || v == 2 ? v : 0;
}
#define MA_FASTX_PIECE_DEFAULT ((size_t)16 << 20)
size_t ma_fastx_piece(void)
{
	const char *s = getenv("MA_FASTX_PIECE");
	long long v = s && *s ? atoll(s) : (long long)MA_FASTX_PIECE_DEFAULT;
	return v < 256 ? (size_t)256 : v > (1ll << 30) ? (size_t)1 << 30 : (size_t)v;
}

/* The reads file through the device a piece at a time (csrc/useq.hip): f->fp is read in pieces of whole lines by a second thread (ingest_gpu.c:
 * ma_stream_q_t) while this one has the piece before uploaded, indexed, checked, looked up and placed.  Returns 1 when the whole input went that way; 0 when
 * a window got a verdict other than OK (ui->reason): the windows before it are placed, and f reads on from the first byte of that
 * window -- the window itself (fetched from the device at this moment only), what the producer had read ahead, then the rest of fp; nothing is read twice.
 * *keep: memory f points into, to be freed behind the host reader.  -1 on an error.  pl == 0: the plan's table, as in ug_seq_device. */
enum { SLAP_PRODUCER, SLAP_UPLOAD, SLAP_INDEX, SLAP_LOOKUP, SLAP_PLACE, SLAP_WAIT, N_SLAPS };
typedef struct { void *window; ma_stream_q_t q; int q_live; fq_pre_t pre; } stream_keep_t;
static int ug_seq_stream(mahip_ctx_t *c, const sdict_t *d, const ma_sub_t *sub, fq_stream_t *f, const utg_place_t *pl, const uint64_t *uoff, size_t piece_bytes, mahip_useq_info_t *ui,
                         mahip_useq_stream_report_t *sr, double *slaps, stream_keep_t *keep)
{
	mahip_useq_want_t *want = 0;
	char *names = 0;
	size_t n_want = 0, name_bytes = 0;
	ma_stream_q_t *q = &keep->q;
	int i = 0, rc, handed = 0;
	if (pl) ug_seq_wanted(d, sub, pl, uoff, &want, &names, &n_want, &name_bytes);
	mahip_mem_trim(c, 0);
	rc = pl ? mahip_useq_stream_begin(c, want, n_want, names, name_bytes) : mahip_useq_stream_begin_planned(c);
	free(want); free(names);
	if (rc != 0) return -1;
	ma_stream_q_init(q, f->fp, piece_bytes);
	keep->q_live = 1;
	if (ma_stream_q_start(q) != 0) { mahip_useq_stream_abort(c); return -1; }
	for (;; i ^= 1) {
		mahip_useq_stream_verdict_t v;
		int last;
		if (ma_stream_q_wait(q, i) != 0) { fprintf(stderr, "[E::%s] out of memory for a piece of the reads file\n", __func__); exit(1); }
		last = q->b[i].last;
		if (mahip_useq_stream_piece_mem(c, q->b[i].p, q->b[i].len, last, &v) != 0) { ma_stream_q_release(q, i, 1); ma_stream_q_join(q); mahip_useq_stream_abort(c); return -1; }
		if (v.reason != MAHIP_FASTX_OK) { /* the handover: never a rewind */
			uint64_t wn = 0;
			ma_stream_q_halt(q); /* b[i] is still ours; b[i ^ 1] holds the next piece if there is one; cut.carry what follows it */
			if (mahip_useq_stream_window_download(c, 0, &wn) != 0) return -1;
			keep->window = malloc(wn ? wn : 1);
			if (mahip_useq_stream_window_download(c, keep->window, &wn) != 0) return -1;
			keep->pre.seg[0].p = (const unsigned char*)keep->window; keep->pre.seg[0].len = (size_t)wn;
			if (!last && q->b[i ^ 1].full) { keep->pre.seg[1].p = (const unsigned char*)q->b[i ^ 1].p; keep->pre.seg[1].len = q->b[i ^ 1].len; }
			keep->pre.seg[2].p = (const unsigned char*)q->cut.carry; keep->pre.seg[2].len = q->cut.carry_len;
			f->pre = &keep->pre;
			ui->reason = v.reason;
			handed = 1;
			break;
		}
		ma_stream_q_release(q, i, 0);
		if (last) { ma_stream_q_join(q); break; }
	}
	if ((handed ? mahip_useq_stream_abort(c) : mahip_useq_stream_end(c)) != 0) return -1;
	mahip_useq_stream_last(c, sr);
	if (mahip_fastx_release(c) != 0) return -1;
	ui->format = sr->format; ui->n_records = sr->n_records; ui->n_matched = sr->n_matched; ui->n_dup = sr->n_dup; ui->n_short = sr->n_short;
	slaps[SLAP_PRODUCER] = q->t_prod * 1e3; slaps[SLAP_WAIT] = q->t_wait * 1e3;
	slaps[SLAP_UPLOAD] = sr->laps_ms[0]; slaps[SLAP_INDEX] = sr->laps_ms[1]; slaps[SLAP_LOOKUP] = sr->laps_ms[2]; slaps[SLAP_PLACE] = sr->laps_ms[3];
	if (!handed) ui->reason = MAHIP_FASTX_OK;
	return handed ? 0 : 1;
}

/* Host reader (the fallback: gzip, stdin, files outside the regular form): the file is read here (one inflate stream, the reference's record rules); the bases of every read that sits on a unitig go to
 * the device in batches and a byte-gather kernel places them (forward copy / reverse complement, csrc/useq.hip); the unitig
 * strings come back once, at the end. */
#define USEQ_BATCH_BYTES ((size_t)256 << 20)
/* the host reader's loop (asm.c:262-284) over what f0 still holds.  The stream is a local copy whose address goes nowhere, so its cursor stays in registers: fq_getc
 * runs once per byte of the input */
static void __attribute__((noinline)) ug_seq_host(mahip_ctx_t *c, const sdict_t *d, const ma_sub_t *sub, const fq_stream_t *f0, const utg_place_t *pl, const uint64_t *uoff)
{
	fq_stream_t f = *f0;
	fq_str_t name = {0, 0, 0}, seq = {0, 0, 0};
	size_t n_jobs = 0, m_jobs = 1 << 16, n_batch = 0, m_batch = USEQ_BATCH_BYTES;
	char *batch = (char*)malloc(m_batch);
	mahip_useq_job_t *jobs = (mahip_useq_job_t*)malloc(m_jobs * sizeof(mahip_useq_job_t));
	uint32_t *in_batch = (uint32_t*)calloc(d->n_seq ? d->n_seq : 1, sizeof(uint32_t)), batch_no = 1; /* the batch that holds a job of the read */
	int last = 0;
	f.buf = (unsigned char*)malloc(FQ_BUF);
	while (fq_read(&f, &last, &name, &seq) >= 0) {
		int32_t id = name.s ? sd_get(d, name.s) : -1;
		const utg_place_t *t;
		const char *rs = seq.s;
		size_t rl = seq.l;
		if (id < 0 || pl[id].len == 0) continue;
		t = &pl[id];
		if (sub) {
			assert(sub[id].e - sub[id].s <= rl);
			rs += sub[id].s; rl = sub[id].e - sub[id].s;
		}
		if (n_batch + rl > m_batch || n_jobs == m_jobs || in_batch[id] == batch_no) { /* batch full: place what is there.  A name the file carries twice: the later record has to win
		                                                                                 * (asm.c:262-284 overwrites), and the jobs of ONE batch run side by side -- it goes into the next */
			GPU(mahip_useq_batch(c, batch, n_batch, jobs, n_jobs));
			n_batch = 0; n_jobs = 0; ++batch_no;
			if (rl > m_batch) { m_batch = rl; batch = (char*)realloc(batch, m_batch); }
		}
		in_batch[id] = batch_no;
		memcpy(batch + n_batch, rs, rl);
		jobs[n_jobs].src_off = n_batch; jobs[n_jobs].dst_off = uoff[t->utg] + t->start;
		jobs[n_jobs].src_len = (uint32_t)rl; jobs[n_jobs].len = t->len; jobs[n_jobs].rev = t->ori; jobs[n_jobs].pad = 0;
		++n_jobs; n_batch += rl;
	}
	GPU(mahip_useq_batch(c, batch, n_batch, jobs, n_jobs));
	free(batch); free(jobs); free(in_batch); free(name.s); free(seq.s); free(f.buf);
}

/* ma_ug_seq in two steps.  ma_ug_seq_place: everything up to the finished arena, which stays in HBM (mahip_useq_end(c, NULL)); -1: the reads file cannot be opened.
 * Then EITHER ma_ug_seq_fetch (the arena comes down and is cut into one string per unitig: what ma_ug_seq always did) OR ma_ug_seq_drop (the device text writer
 * took the bases from the arena: nothing comes down).  Both print the timing line and free the job. */
struct ma_ug_seq_job {
	mahip_ctx_t *c;
	fq_stream_t f;
	uint64_t *uoff, tot;
	int on_device, streamed;
	size_t piece_bytes;
	mahip_useq_info_t ui;
	mahip_useq_stream_report_t sr;
	stream_keep_t keep;
	double laps[N_LAPS], slaps[N_SLAPS];
};

/* the job with its reads file open (opened before anything else, as the reference does: a missing file is an error, not a fallback; nothing is read through it
 * unless the host reader runs); 0: it cannot be opened */
static ma_ug_seq_job_t *ug_seq_open(const char *fn)
{
	ma_ug_seq_job_t *q = (ma_ug_seq_job_t*)calloc(1, sizeof(ma_ug_seq_job_t));
	q->piece_bytes = ma_fastx_piece();
	q->f.fp = fn && strcmp(fn, "-") ? gzopen(fn, "r") : gzdopen(fileno(stdin), "r");
	if (q->f.fp == 0) { free(q); return 0; }
	return q;
}

/* the plan of the context to the host, as the host reader wants it: pl[d->n_seq], q->uoff (asm.c:248-260, computed by mahip_useq_plan) */
static utg_place_t *ug_seq_plan_fetch(ma_ug_seq_job_t *q, const sdict_t *d)
{
	mahip_useq_plan_info_t pi;
	mahip_useq_place_t *dl;
	utg_place_t *pl = (utg_place_t*)calloc(d->n_seq ? d->n_seq : 1, sizeof(utg_place_t));
	uint32_t i;
	mahip_useq_plan_last(q->c, &pi);
	if (pi.n_reads != d->n_seq) { fprintf(stderr, "[E::%s] the plan describes %llu reads, the dictionary %u\n", __func__, (unsigned long long)pi.n_reads, d->n_seq); exit(1); }
	dl = (mahip_useq_place_t*)malloc((d->n_seq ? d->n_seq : 1) * sizeof(mahip_useq_place_t));
	if (q->uoff == 0) q->uoff = (uint64_t*)malloc((pi.n_utg + 1) * 8);
	GPU(mahip_useq_plan_download(q->c, q->uoff, dl, 0, 0));
	for (i = 0; i < d->n_seq; ++i) pl[i].utg = dl[i].utg, pl[i].ori = dl[i].ori, pl[i].start = dl[i].start, pl[i].len = dl[i].len;
	free(dl);
	return pl;
}

/* the three readers in their order under their switches (MA_FASTX_HOST, MA_FASTX_STREAM, MA_FASTX_PIECE) behind mahip_useq_begin, up to the finished arena.
 * pl == 0: the plan is the context's (ma_ug_seq_place_planned) -- the device readers take its table where it lies, the host reader brings pl and uoff down */
static void ug_seq_readers(ma_ug_seq_job_t *q, const sdict_t *d, const ma_sub_t *sub, const char *fn, utg_place_t *pl)
{
	mahip_ctx_t *c = q->c;
	const int stream_mode = ma_fastx_stream_mode();
	int forced, streamed = 0, on_device = 0;
	{ const char *e = getenv("MA_FASTX_HOST"); forced = e && atoi(e) != 0; }
	if (forced || stream_mode != 2) { /* the whole-file device reader first, as ever */
		on_device = ug_seq_device(c, d, sub, fn, pl, q->uoff, &q->ui, q->laps);
		if (on_device < 0) ma_gpu_fail(__func__);
	}
	if (!forced && !on_device && (stream_mode == 2 || (stream_mode == 1 && (q->ui.reason == MAHIP_FASTX_NOT_PLAIN || q->ui.reason == MAHIP_FASTX_NOMEM)))) { /* the streamed device reader */
		memset(&q->ui, 0, sizeof(q->ui));
		streamed = 1;
		on_device = ug_seq_stream(c, d, sub, &q->f, pl, q->uoff, q->piece_bytes, &q->ui, &q->sr, q->slaps, &q->keep);
		if (on_device < 0) ma_gpu_fail(__func__);
	}
	q->ui.reader = streamed ? MAHIP_USEQ_STREAM : on_device ? MAHIP_USEQ_DEVICE : MAHIP_USEQ_HOST;
	mahip_useq_note(c, &q->ui);
	if (!on_device) {
		utg_place_t *own = 0;
		if (streamed) fprintf(stderr, "[W::%s] reads file handed to the host reader at piece %lld: %s\n", "ma_ug_seq", (long long)q->sr.refused_piece, mahip_fastx_reason_name(q->ui.reason));
		else fprintf(stderr, "[W::%s] reads file read on the host: %s\n", "ma_ug_seq", mahip_fastx_reason_name(q->ui.reason));
		if (pl == 0) pl = own = ug_seq_plan_fetch(q, d);
		ug_seq_host(c, d, sub, &q->f, pl, q->uoff);
		free(own);
	}
	GPU(mahip_useq_end(c, 0)); /* finished; it stays in HBM */
	q->on_device = on_device; q->streamed = streamed;
}

int ma_ug_seq_place(ma_ug_t *g, const sdict_t *d, const ma_sub_t *sub, const char *fn, ma_ug_seq_job_t **job)
{
	ma_ug_seq_job_t *q = ug_seq_open(fn);
	mahip_ctx_t *c;
	utg_place_t *pl;
	uint64_t *uoff, tot = 0;
	uint32_t i, j;
	*job = 0;
	if (q == 0) return -1;
	c = q->c = ma_gpu();
	pl = (utg_place_t*)calloc(d->n_seq ? d->n_seq : 1, sizeof(utg_place_t));
	uoff = q->uoff = (uint64_t*)malloc((g->u.n + 1) * 8);
	for (i = 0; i < g->u.n; ++i) { /* where every read lands; unitig strings back to back, each with its terminator */
		const ma_utg_t *u = &g->u.a[i];
		uint32_t l = 0;
		uoff[i] = tot; tot += (uint64_t)u->len + 1;
		for (j = 0; j < u->n; ++j) {
			utg_place_t *t = &pl[u->a[j] >> 33];
			assert(t->len == 0);
			t->utg = i, t->ori = u->a[j] >> 32 & 1;
			t->start = l, t->len = (uint32_t)u->a[j];
			l += t->len;
		}
	}
	q->tot = tot;
	GPU(mahip_useq_begin(c, (size_t)tot));
	ug_seq_readers(q, d, sub, fn, pl);
	free(pl);
	*job = q;
	return 0;
}

/* ma_ug_seq_place without ma_ug_t: the plan (asm.c:248-260 and the wanted table) is made on the device from the unitigs mahip_ug_gen left in c, the names of
 * mahip_text_names and the kept intervals (mahip_useq_plan; no member word comes down), then the same readers run.  0: placed; -1: the reads file cannot be opened
 * (the plan stays, nothing is placed); 1: the plan was refused (pi->reason; nothing in the context changed, the caller takes ma_ug_seq_place).  d: the dictionary the names
 * describe, with its index (the host reader looks names up in it).  Then ma_ug_seq_drop, or ma_ug_seq_fetch with a ma_ug_t unpacked for it. */
int ma_ug_seq_place_planned(mahip_ctx_t *c, const sdict_t *d, const ma_sub_t *sub, const char *fn, mahip_useq_plan_info_t *pi, ma_ug_seq_job_t **job)
{
	ma_ug_seq_job_t *q;
	*job = 0;
	memset(pi, 0, sizeof(*pi));
	GPU(mahip_useq_plan(c, sub != 0, pi)); /* (before the file is opened: a refusal leaves it, stdin included, to ma_ug_seq_place) */
	if (pi->road != MAHIP_PLAN_ROAD_DEVICE) return 1;
	if ((q = ug_seq_open(fn)) == 0) return -1;
	q->c = c;
	q->tot = pi->arena_bytes;
	GPU(mahip_useq_begin_planned(c));
	ug_seq_readers(q, d, sub, fn, 0);
	*job = q;
	return 0;
}

static void ug_seq_close(ma_ug_seq_job_t *q)
{
	static const char *const fmt_name[] = {"?", "fasta", "fastq"};
	const mahip_useq_info_t ui = q->ui;
	const mahip_useq_stream_report_t sr = q->sr;
	const double *laps = q->laps, *slaps = q->slaps;
	if (ma_timing_level() >= 1) {
		if (q->streamed) {
			char ho[32];
			if (sr.refused_piece < 0) strcpy(ho, "none"); else snprintf(ho, sizeof(ho), "%lld", (long long)sr.refused_piece);
			fprintf(stderr, "[T::ug_seq] reader=stream format=%s pieces=%llu piece=%llu B records=%llu matched=%llu dup=%llu handover=%s reason=%d : producer %.3f upload %.3f index %.3f lookup %.3f place %.3f waited-for-input %.3f download %.3f ms\n",
			        fmt_name[ui.format], (unsigned long long)sr.n_pieces, (unsigned long long)q->piece_bytes, (unsigned long long)ui.n_records, (unsigned long long)ui.n_matched, (unsigned long long)ui.n_dup, ho, ui.reason,
			        slaps[SLAP_PRODUCER], slaps[SLAP_UPLOAD], slaps[SLAP_INDEX], slaps[SLAP_LOOKUP], slaps[SLAP_PLACE], slaps[SLAP_WAIT], laps[LAP_DOWNLOAD]);
		} else if (q->on_device) fprintf(stderr, "[T::ug_seq] reader=device format=%s records=%llu matched=%llu dup=%llu : load %.3f index %.3f lookup %.3f place %.3f download %.3f ms\n", fmt_name[ui.format],
		                       (unsigned long long)ui.n_records, (unsigned long long)ui.n_matched, (unsigned long long)ui.n_dup, laps[LAP_LOAD], laps[LAP_INDEX], laps[LAP_LOOKUP], laps[LAP_PLACE], laps[LAP_DOWNLOAD]);
		else fprintf(stderr, "[T::ug_seq] reader=host reason=%d format=%s records=%llu : download %.3f ms\n", ui.reason, fmt_name[ui.format], (unsigned long long)ui.n_records, laps[LAP_DOWNLOAD]);
	}
	free(q->uoff);
	if (q->keep.q_live) ma_stream_q_destroy(&q->keep.q);
	free(q->keep.window);
	if (q->f.fp) gzclose(q->f.fp);
	free(q);
}

mahip_ctx_t *ma_ug_seq_ctx(const ma_ug_seq_job_t *q) { return q->c; }

void ma_ug_seq_drop(ma_ug_seq_job_t *q) { ug_seq_close(q); }

void ma_ug_seq_fetch(ma_ug_t *g, ma_ug_seq_job_t *q)
{
	char *arena = (char*)malloc(q->tot ? q->tot : 1);
	const double t_dl = sys_realtime();
	uint32_t i;
	GPU(mahip_useq_end(q->c, arena));
	if (q->uoff == 0) { /* a planned placement whose host reader did not run: where the strings start is still on the device alone */
		q->uoff = (uint64_t*)malloc(((size_t)g->u.n + 1) * 8);
		GPU(mahip_useq_plan_download(q->c, q->uoff, 0, 0, 0));
	}
	q->laps[LAP_DOWNLOAD] = (sys_realtime() - t_dl) * 1e3;
	for (i = 0; i < g->u.n; ++i) { /* ma_ug_destroy frees every string on its own */
		ma_utg_t *u = &g->u.a[i];
		u->s = (char*)malloc((size_t)u->len + 1);
		memcpy(u->s, arena + q->uoff[i], u->len);
		u->s[u->len] = 0;
	}
	free(arena);
	ug_seq_close(q);
}

int ma_ug_seq(ma_ug_t *g, const sdict_t *d, const ma_sub_t *sub, const char *fn)
{
	ma_ug_seq_job_t *q;
	if (ma_ug_seq_place(g, d, sub, fn, &q) != 0) return -1;
	ma_ug_seq_fetch(g, q);
	return 0;
}
