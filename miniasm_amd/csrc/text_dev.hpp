// text_dev.hpp -- the text of the three record dumps (-p paf, -p sg, -p bed) and of the unitig GFA (-p ug, with -f sequences) written on the device: kernels and
// the entries of include/mahip.h behind them.
// A header, included by exactly one translation unit (mahip_api.hip).  The per-line arithmetic is text_core.h's, shared with the host tests.
//
// Per slab of records:  k_text_len (one length per record)  ->  scan_exclusive_u32 (where each line starts; u32, so a slab's text stays below 2^32 bytes)
// ->  k_text_write.  The write kernel gives a wave 64 consecutive records, whose lines are one contiguous stretch of the text.  Every lane formats its line into
// the wave's LDS tile at its place in that stretch; the tile is laid out with the stretch's misalignment in front, so that 16-byte-aligned addresses of the text are
// 16-byte-aligned offsets of the tile, and the wave streams it out with 16-byte stores (the bytes in front of the first and behind the last aligned address go
// singly).  A stretch that does not fit the tile -- a name of tens of kilobytes -- takes the slow path: its lanes write byte by byte straight to the text.
#pragma once
#include "mahip_internal.hpp"
#include "text_core.h"

#ifndef MA_TEXT_TILE
#define MA_TEXT_TILE 12288u // bytes of LDS per wave (one wave per block): 64 lines of 190 bytes; 13 blocks per CU
#endif
#define MA_TEXT_SLAB_DEFAULT (4ull << 20) // records per slab unless MA_TEXT_SLAB says otherwise
// bases per chunk record of an S line (-p ug -f): a wave of 64 chunk records is 8 KiB, which leaves 4 KiB of the tile to the lines of a mixed wave, and the default slab
// of 4 Mi records of at most max(MA_TEXT_SEQ_CHUNK, TC_FIXED_UG + 2 names) bytes stays below 2^32 bytes for names up to 450 bytes
#ifndef MA_TEXT_SEQ_CHUNK
#define MA_TEXT_SEQ_CHUNK 128u
#endif

struct TextIn { int kind; const uint32_t *rec; const uint32_t *sub; const uint8_t *del; const char *blob; const uint64_t *off; tc_ug_t ug; };

// record r through the emitter; returns the '\n' bytes of the record
__device__ __forceinline__ uint32_t text_record(tc_emit_t *e, const TextIn &in, uint64_t r, const tc_names_t *nm)
{
	if (in.kind == TC_KIND_UG) return tc_line_ug(e, &in.ug, r, nm, in.sub);
	tc_line(e, in.kind, r, in.rec, nm, in.sub, in.del);
	return e->n != 0;
}

// len[i] = bytes of record r0 + i; ctr[0] += the lines they hold (a record dump: records that are not empty; the unitig GFA: '\n' bytes)
__global__ __launch_bounds__(256) void k_text_len(TextIn in, uint64_t r0, uint32_t cnt, uint32_t *__restrict__ len, unsigned long long *ctr)
{
	const tc_names_t nm = {in.blob, in.off};
	uint64_t lines = 0;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
		tc_emit_t e = {nullptr, 0};
		lines += text_record(&e, in, r0 + i, &nm);
		len[i] = e.n;
	}
	blk_add_u64(ctr, lines);
}

// start[0 .. cnt]: where the lines of records r0 .. r0 + cnt begin in text (start[cnt] = all of it).  One wave per block, 64 records per wave.
__global__ __launch_bounds__(64) void k_text_write(TextIn in, uint64_t r0, uint32_t cnt, const uint32_t *__restrict__ start, char *text, unsigned long long *ctr)
{
	__shared__ __attribute__((aligned(16))) char s_tile[MA_TEXT_TILE];
	const tc_names_t nm = {in.blob, in.off};
	const uint32_t lane = threadIdx.x, first = blockIdx.x * 64u, last = first + 64u < cnt ? first + 64u : cnt;
	const uint32_t s0 = start[first], span = start[last] - s0;
	if (span == 0) return; // (the whole wave: a bed dump skips reads)
	const uint32_t i = first + lane;
	const bool have = i < cnt;
	const uint32_t my = have ? start[i] : 0, my_len = have ? start[i + 1] - my : 0;
	char *g = text + s0;
	const uint32_t pad = (uint32_t)((uintptr_t)g & 15u);
	if (pad + span <= MA_TEXT_TILE) {
		if (my_len) {
			tc_emit_t e = {s_tile + pad + (my - s0), 0};
			text_record(&e, in, r0 + i, &nm);
		}
		__syncthreads();
		uint32_t head = (16u - pad) & 15u; // bytes in front of the first aligned address
		if (head > span) head = span;
		if (lane < head) g[lane] = s_tile[pad + lane];
		const uint32_t nvec = (span - head) >> 4;
		const uint4 *src = (const uint4*)(s_tile + pad + head);
		uint4 *dst = (uint4*)(g + head);
		for (uint32_t v = lane; v < nvec; v += 64u) dst[v] = src[v];
		const uint32_t done = head + (nvec << 4); // fewer than 16 bytes are left
		if (lane < span - done) g[done + lane] = s_tile[pad + done + lane];
	} else { // the slow path
		if (my_len) {
			tc_emit_t e = {text + my, 0};
			text_record(&e, in, r0 + i, &nm);
		}
		wv_count_add(ctr + 1, my_len != 0);
	}
}

// tot[s] = bytes of slab s (the scan left them behind the slab's starts)
__global__ __launch_bounds__(256) void k_text_totals(const uint32_t *__restrict__ start, uint64_t stride, uint64_t n, uint64_t slab, uint32_t n_slabs, uint32_t *__restrict__ tot)
{
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= n_slabs) return;
	const uint64_t r0 = (uint64_t)s * slab, cnt = n - r0 < slab ? n - r0 : slab;
	tot[s] = start[(uint64_t)s * stride + cnt];
}

// kept intervals in the squeezed numbering (hits.hip: k_sub_squeeze does the same for mahip_sub_download)
__global__ __launch_bounds__(256) void k_text_sub_squeeze(const uint2 *__restrict__ sub, const int32_t *__restrict__ map, uint32_t n_seq, uint2 *__restrict__ out)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < n_seq && map[r] >= 0) out[map[r]] = sub[r];
}

// ---- the unitig GFA: what the record space of text_core.h: tc_ug_t needs beside the unitigs themselves
// cnt[i] = records unitig i owns in the units block (chunk == 0: no sequences); ctr[2] += their sum in 64 bits
__global__ __launch_bounds__(256) void k_text_ug_count(const uint32_t *__restrict__ u_n, const uint32_t *__restrict__ u_len, uint32_t U, uint32_t chunk, uint32_t *__restrict__ cnt, unsigned long long *ctr)
{
	uint64_t sum = 0;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < U; i += (size_t)gridDim.x * 256) {
		const uint32_t len = u_len[i];
		const uint64_t k = 1ull + u_n[i] + (chunk ? 1ull + len / chunk + (len % chunk != 0) : 0ull);
		cnt[i] = (uint32_t)k;
		sum += k;
	}
	blk_add_u64(ctr + 2, sum);
}

// low[m] = the low word of member m: its length contribution, summed up (mod 2^32) by the scan into the reference's l
__global__ __launch_bounds__(256) void k_text_ug_low(const uint64_t *__restrict__ mem, uint32_t M, uint32_t *__restrict__ low)
{
	for (size_t m = (size_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (size_t)gridDim.x * 256) low[m] = (uint32_t)mem[m];
}

// low[] and its scan for the members of a set of unitigs: what tc_ug_member_start reads, for the `a` lines and for the placement plan (useq.hip)
int text_ug_member_scan(mahip_ctx *c, const uint64_t *mem, uint32_t M, uint32_t *low, uint32_t *mscan)
{
	hipLaunchKernelGGL(k_text_ug_low, dim3(grid_for(M, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, mem, M, low);
	HIPCHK(hipGetLastError());
	return scan_exclusive_u32(c, low, mscan, M, nullptr);
}

// ctr[3] += 8-byte words (single bytes in front of the first and behind the last aligned address) of a[0 .. n) that hold a NUL byte
__global__ __launch_bounds__(256) void k_text_count_nul(const char *__restrict__ a, uint64_t n, unsigned long long *ctr)
{
	uint64_t head = (8u - (uint32_t)((uintptr_t)a & 7u)) & 7u, found = 0;
	if (head > n) head = n;
	const uint64_t nw = (n - head) >> 3, done = head + (nw << 3);
	const uint64_t *w = (const uint64_t*)(a + head);
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * 256) {
		const uint64_t x = w[i];
		found += ((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull) != 0;
	}
	if (blockIdx.x == 0) {
		if (threadIdx.x < head) found += a[threadIdx.x] == 0;
		if (threadIdx.x < n - done) found += a[done + threadIdx.x] == 0;
	}
	blk_add_u64(ctr + 3, found);
}

// ================================================================================================ host side

struct TextState {
	DevBuf blob, off, del, sub, rec, len, start, tot, ctr, txt[2];
	DevBuf ug_cnt, ug_rbase, ug_moff, ug_low, ug_mscan, ug_links, ug_ecnt, ug_uoff;          // the record space of the unitig GFA
	DevBuf ug_un, ug_ulen, ug_ustart, ug_uend, ug_mem, ug_arena;                              // hand-made unitigs of the stage entry
	char *host[2] = {nullptr, nullptr};
	size_t host_cap[2] = {0, 0};
	hipEvent_t ev[2][2] = {};
	bool ev_ready = false;
	uint32_t n_seq = 0;
	uint64_t max_name = 0, names_bytes = 0;
	bool names = false, has_del = false;
	uint64_t names_gen = 0; // mahip_text_names calls so far: the placement plan's table points into the blob (useq.hip)
	double names_ms = 0;
	// what prepare left for emit
	bool planned = false;
	TextIn in = {};
	uint64_t n = 0, slab = 0, n_slabs = 0, stride = 0;
	std::vector<uint32_t> tot_h;
	mahip_text_info_t last = {};
};

static TextState *text_of(mahip_ctx *c) { if (!c->text) c->text = new TextState(); return (TextState*)c->text; }

void text_free(mahip_ctx *c)
{
	TextState *t = (TextState*)c->text;
	if (!t) return;
	DevBuf *all[] = {&t->blob, &t->off, &t->del, &t->sub, &t->rec, &t->len, &t->start, &t->tot, &t->ctr, &t->txt[0], &t->txt[1],
	                 &t->ug_cnt, &t->ug_rbase, &t->ug_moff, &t->ug_low, &t->ug_mscan, &t->ug_links, &t->ug_ecnt, &t->ug_uoff,
	                 &t->ug_un, &t->ug_ulen, &t->ug_ustart, &t->ug_uend, &t->ug_mem, &t->ug_arena};
	for (DevBuf *b : all) dev_free(c, *b);
	for (int k = 0; k < 2; ++k) { free(t->host[k]); for (int e = 0; e < 2; ++e) if (t->ev[k][e]) (void)hipEventDestroy(t->ev[k][e]); }
	delete t;
	c->text = nullptr;
}

extern "C" int mahip_text_enabled(void)
{
	const char *e = getenv("MA_TEXT_DEVICE");
	return e && atoi(e) != 0; // unset: off.  Measured against the parent commit: -p paf -S2 on the 40 M-line stand-in 2.9 s against 21.7 s, but -p sg -S5 (24 MB of text) within the parent's own spread -- the rule asked for both
}

static uint64_t text_slab_default()
{
	const char *e = getenv("MA_TEXT_SLAB");
	const long long v = e ? atoll(e) : 0;
	return v > 0 ? (uint64_t)v : MA_TEXT_SLAB_DEFAULT;
}

extern "C" int mahip_text_names(mahip_ctx_t *c, const char *blob, const uint64_t *off, uint32_t n_seq, const uint8_t *del)
{
	HIPCHK(hipSetDevice(c->dev));
	TextState *t = text_of(c);
	const double t0 = TieLaps::now();
	t->names = false; ++t->names_gen;
	const uint64_t bytes = n_seq ? off[n_seq] : 0;
	uint64_t mx = 0;
	for (uint32_t i = 0; i < n_seq; ++i) { const uint64_t l = off[i + 1] - off[i]; if (l > mx) mx = l; }
	CHK(dev_reserve(c, t->blob, bytes + 16));
	CHK(dev_reserve(c, t->off, ((size_t)n_seq + 2) * 8));
	if (bytes) CHK(xfer_copy(c, t->blob.p, (void*)blob, bytes, 1));
	if (n_seq) CHK(xfer_copy(c, t->off.p, (void*)off, ((size_t)n_seq + 1) * 8, 1));
	t->has_del = del != nullptr && n_seq != 0;
	if (t->has_del) {
		CHK(dev_reserve(c, t->del, (size_t)n_seq + 16));
		CHK(xfer_copy(c, t->del.p, (void*)del, n_seq, 1));
	}
	t->n_seq = n_seq; t->max_name = mx; t->names_bytes = bytes; t->names = true;
	t->names_ms = (TieLaps::now() - t0) * 1e3;
	return 0;
}

static void text_info_begin(TextState *t, int kind, mahip_text_info_t *info)
{
	memset(info, 0, sizeof(*info));
	info->kind = kind; info->road = MAHIP_TEXT_ROAD_HOST; info->max_name = t->max_name;
	info->laps_ms[0] = t->names_ms;
}

static int text_host_road(TextState *t, mahip_text_info_t *info, int reason, const char *why)
{
	info->road = MAHIP_TEXT_ROAD_HOST; info->reason = reason;
	t->planned = false; t->last = *info;
	mahip_set_error("device text writer not used: %s", why); // (not an error: the caller's log line names the reason)
	return 0;
}

// lengths and starts of every slab, the slabs' byte counts on the host, the text buffers: after this nothing can fail but a copy or the sink
static int text_plan(mahip_ctx *c, TextState *t, int kind, const uint32_t *d_rec, uint64_t n, const uint32_t *d_sub, uint64_t slab_req, mahip_text_info_t *info)
{
	const double t0 = TieLaps::now();
	const uint64_t fixed = kind == MAHIP_TEXT_PAF ? TC_FIXED_PAF : kind == MAHIP_TEXT_SG ? TC_FIXED_SG : kind == MAHIP_TEXT_UG ? TC_FIXED_UG : TC_FIXED_BED;
	uint64_t max_line = fixed + (kind == MAHIP_TEXT_BED ? 1 : 2) * t->max_name;
	if (kind == MAHIP_TEXT_UG && t->in.ug.arena && max_line < t->in.ug.chunk) max_line = t->in.ug.chunk; // (a chunk record)
	uint64_t slab = slab_req ? slab_req : text_slab_default();
	if (slab > 0xffffffffull / max_line) slab = 0xffffffffull / max_line; // records x longest possible line < 2^32: the scan and the starts are u32
	if (slab > 0x7fffffffull) slab = 0x7fffffffull;
	if (slab < 1) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "a single line may pass 4 GiB");
	const uint64_t n_slabs = (n + slab - 1) / slab, most = n < slab ? n : slab, stride = (most + 1 + 3) & ~3ull; // (16-byte rows: the scan loads uint4)
	t->in.kind = kind; t->in.rec = d_rec; t->in.sub = d_sub; t->in.del = t->has_del ? (const uint8_t*)t->del.p : nullptr;
	t->in.blob = (const char*)t->blob.p; t->in.off = (const uint64_t*)t->off.p;
	t->n = n; t->slab = slab; t->n_slabs = n_slabs; t->stride = stride;
	t->tot_h.assign(n_slabs + 1, 0);
	uint64_t n_lines = 0, total = 0, max_tot = 0;
	if (dev_reserve(c, t->ctr, 64) != 0) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the counters");
	HIPCHK(hipMemsetAsync(t->ctr.p, 0, 64, c->st));
	if (n_slabs) {
		if (dev_reserve(c, t->len, (stride + 16) * 4) != 0 || dev_reserve(c, t->start, (n_slabs * stride + 16) * 4) != 0 || dev_reserve(c, t->tot, (n_slabs + 16) * 4) != 0)
			return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the line lengths");
		for (uint64_t s = 0; s < n_slabs; ++s) {
			const uint64_t r0 = s * slab;
			const uint32_t cnt = (uint32_t)(n - r0 < slab ? n - r0 : slab);
			uint32_t *start = P<uint32_t>(t->start) + s * stride;
			hipLaunchKernelGGL(k_text_len, dim3(grid_for(cnt, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, t->in, r0, cnt, P<uint32_t>(t->len), P<unsigned long long>(t->ctr));
			CHK(scan_exclusive_u32(c, P<uint32_t>(t->len), start, cnt, start + cnt));
		}
		hipLaunchKernelGGL(k_text_totals, dim3(grid_for(n_slabs, 256)), dim3(256), 0, c->st, (const uint32_t*)P<uint32_t>(t->start), stride, n, slab, (uint32_t)n_slabs, P<uint32_t>(t->tot));
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(t->tot_h.data(), t->tot.p, n_slabs * 4, hipMemcpyDeviceToHost, c->st));
	}
	unsigned long long h_ctr[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(h_ctr, t->ctr.p, 16, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	n_lines = h_ctr[0];
	for (uint64_t s = 0; s < n_slabs; ++s) { total += t->tot_h[s]; if (t->tot_h[s] > max_tot) max_tot = t->tot_h[s]; }
	for (int k = 0; k < 2 && (uint64_t)k < n_slabs; ++k) {
		if (max_tot == 0) break;
		if (dev_reserve(c, t->txt[k], max_tot + 16) != 0) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the text of a slab");
		if (t->host_cap[k] < max_tot) {
			char *p = (char*)realloc(t->host[k], max_tot);
			if (!p) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no host memory for the text of a slab");
			t->host[k] = p; t->host_cap[k] = max_tot;
		}
	}
	if (!t->ev_ready) {
		for (int k = 0; k < 2; ++k) for (int e = 0; e < 2; ++e) HIPCHK(hipEventCreate(&t->ev[k][e]));
		t->ev_ready = true;
	}
	info->road = MAHIP_TEXT_ROAD_DEVICE; info->reason = MAHIP_TEXT_OK;
	info->n_records = n; info->n_lines = n_lines; info->text_bytes = total; info->n_slabs = n_slabs; info->slab_records = slab;
	info->laps_ms[2] = (TieLaps::now() - t0) * 1e3;
	t->planned = true; t->last = *info;
	return 0;
}

// kept intervals of slot 0 in the numbering the records use (squeezed when a squeeze map is pending), as mahip_sub_download hands them over; 1: no device memory
static int text_sub_export(mahip_ctx *c, TextState *t, uint32_t Rn, const uint32_t **d_sub)
{
	if (dev_reserve(c, t->sub, ((size_t)(c->n_seq > Rn ? c->n_seq : Rn) + 2) * 8) != 0) return 1;
	if (c->has_map) {
		if (c->n_seq) hipLaunchKernelGGL(k_text_sub_squeeze, dim3(grid_for(c->n_seq, 256)), dim3(256), 0, c->st, (const uint2*)P<uint2>(c->sub[0]), (const int32_t*)P<int32_t>(c->map), c->n_seq, P<uint2>(t->sub));
	} else if (c->n_seq) HIPCHK(hipMemcpyAsync(t->sub.p, c->sub[0].p, (size_t)c->n_seq * 8, hipMemcpyDeviceToDevice, c->st));
	*d_sub = P<uint32_t>(t->sub);
	return 0;
}

// ---- what the placement plan (useq.hip) reads of the writer's state: the names as they lie on the device, the kept intervals as the records see them
bool text_dev_names(mahip_ctx *c, const char **blob, const uint64_t **off, uint32_t *n_seq, uint64_t *blob_bytes, uint64_t *gen)
{
	TextState *t = (TextState*)c->text;
	if (gen) *gen = t ? t->names_gen : 0;
	if (!t || !t->names) return false;
	*blob = (const char*)t->blob.p; *off = (const uint64_t*)t->off.p; *n_seq = t->n_seq; *blob_bytes = t->names_bytes;
	return true;
}
int text_dev_sub(mahip_ctx *c, uint32_t Rn, const uint32_t **d_sub) { return text_sub_export(c, text_of(c), Rn, d_sub); }

extern "C" int mahip_text_prepare(mahip_ctx_t *c, int kind, int have_sub, mahip_text_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	TextState *t = text_of(c);
	mahip_text_info_t tmp;
	if (!info) info = &tmp;
	text_info_begin(t, kind, info);
	if (kind == MAHIP_TEXT_UG) { mahip_set_error("mahip_text_prepare: the unitig GFA is prepared by mahip_text_prepare_ug (it takes the sorted unitig arcs)"); return -1; }
	if (kind != MAHIP_TEXT_PAF && kind != MAHIP_TEXT_SG && kind != MAHIP_TEXT_BED) { mahip_set_error("mahip_text_prepare: unknown kind %d", kind); return -1; }
	if (!mahip_text_enabled()) return text_host_road(t, info, MAHIP_TEXT_SWITCHED_OFF, "MA_TEXT_DEVICE is not 1");
	const uint32_t Rn = c->has_map ? c->n_seq_new : c->n_seq; // reads of the numbering the records use (mahip_n_seq_new)
	if (!t->names || (kind != MAHIP_TEXT_SG && t->n_seq != Rn)) return text_host_road(t, info, MAHIP_TEXT_NO_NAMES, "the names on the device do not describe these reads");
	const double t0 = TieLaps::now();
	const uint32_t *d_sub = nullptr;
	if (have_sub) { // slot 0, as mahip_sub_download hands it over
		const int rc = text_sub_export(c, t, Rn, &d_sub);
		if (rc < 0) return -1;
		if (rc > 0) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the kept intervals");
	}
	uint64_t n = 0;
	const uint32_t *d_rec = nullptr;
	if (kind == MAHIP_TEXT_PAF) {
		if (have_sub) { // (main.c:21: without kept intervals a hit dump is empty)
			size_t n_live = 0;
			CHK(hits_export_dev(c, &n_live));
			HIPCHK(hipStreamSynchronize(c->st));
			walk_scratch_release(c);
			n = n_live; d_rec = P<uint32_t>(c->key[0]);
		}
	} else if (kind == MAHIP_TEXT_SG) {
		size_t n_arc = 0;
		uint32_t gR = 0;
		CHK(asg_export_dev(c, &n_arc, &gR, nullptr, nullptr));
		if (gR != t->n_seq) { mahip_set_error("mahip_text_prepare: the graph has %u reads, the names describe %u", gR, t->n_seq); return -1; }
		n = n_arc; d_rec = P<uint32_t>(c->key[0]);
	} else n = have_sub ? t->n_seq : 0; // (main.c:13: no intervals, no bed lines)
	HIPCHK(hipGetLastError());
	if (ma_timing_level() >= 2) HIPCHK(hipStreamSynchronize(c->st));
	info->laps_ms[1] = (TieLaps::now() - t0) * 1e3;
	return text_plan(c, t, kind, d_rec, n, d_sub, 0, info);
}

// ---- the unitig GFA
// unitigs on the device (moff == 0: computed here from u_n), the arena (0: none), both as the caller holds them
// plan_uoff: where every unitig's bases start, on the device already -- the placement plan of these unitigs (useq.hip); 0: made here
struct TextUgSrc { uint32_t U, M; const uint32_t *u_n, *u_len, *u_start, *u_end, *moff; const uint64_t *mem; const char *arena; uint64_t arena_bytes; const uint64_t *plan_uoff; uint64_t plan_tot; };

// links: the unitig arcs in the reference's order (host); counts: 2 U words, arcs leaving each unitig end (host; 0: counted here from the links).  The record space of
// text_core.h: tc_ug_t is built on the device, the refusals are decided, then text_plan runs as for every kind
static int text_plan_ug(mahip_ctx *c, TextState *t, const TextUgSrc &s, const asg_arc_t *links, uint32_t n_links, const uint32_t *counts, const uint32_t *d_sub, int with_seq, uint64_t slab_req,
                        mahip_text_info_t *info)
{
	const double t0 = TieLaps::now();
	const uint32_t U = s.U, M = s.M;
	info->seq_chunk = MA_TEXT_SEQ_CHUNK;
	std::vector<uint64_t> uoff;
	if (with_seq && s.plan_uoff) { // where every unitig's bases start: the plan that placed them holds it
		if (!s.arena || s.arena_bytes != s.plan_tot) return text_host_road(t, info, MAHIP_TEXT_NO_SEQ, "sequences were asked for, but this context holds no finished arena of these unitigs");
		info->n_seq_bytes = s.plan_tot - U;
	} else if (with_seq) { // no plan: the lengths come down (4 U bytes), the offsets go up
		std::vector<uint32_t> len(U);
		uint64_t tot = 0;
		if (U) HIPCHK(hipMemcpyAsync(len.data(), s.u_len, (size_t)U * 4, hipMemcpyDeviceToHost, c->st));
		HIPCHK(hipStreamSynchronize(c->st));
		uoff.resize((size_t)U + 1);
		for (uint32_t i = 0; i < U; ++i) { uoff[i] = tot; tot += (uint64_t)len[i] + 1; }
		uoff[U] = tot;
		if (!s.arena || s.arena_bytes != tot) return text_host_road(t, info, MAHIP_TEXT_NO_SEQ, "sequences were asked for, but this context holds no finished arena of these unitigs");
		info->n_seq_bytes = tot - U;
	}
	std::vector<uint32_t> cnt_h;
	if (!counts) { // asg_arc_n of the cleaned unitig graph
		cnt_h.assign((size_t)2 * U + 1, 0);
		for (uint32_t k = 0; k < n_links; ++k) { const uint64_t v = links[k].ul >> 32; if (v < 2ull * U) ++cnt_h[v]; }
		counts = cnt_h.data();
	}
	DevBuf *w4[] = {&t->ug_cnt, &t->ug_rbase, &t->ug_moff};
	for (DevBuf *b : w4) if (dev_reserve(c, *b, ((size_t)U + 16) * 4) != 0) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the unitigs' record offsets");
	if (dev_reserve(c, t->ug_low, ((size_t)M + 16) * 4) != 0 || dev_reserve(c, t->ug_mscan, ((size_t)M + 16) * 4) != 0 || dev_reserve(c, t->ug_links, ((size_t)n_links + 1) * 16) != 0 ||
	    dev_reserve(c, t->ug_ecnt, ((size_t)2 * U + 16) * 4) != 0 || dev_reserve(c, t->ug_uoff, ((size_t)U + 2) * 8) != 0 || dev_reserve(c, t->ctr, 64) != 0)
		return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the record space of the unitig GFA");
	unsigned long long *ctr = P<unsigned long long>(t->ctr);
	HIPCHK(hipMemsetAsync(t->ctr.p, 0, 64, c->st));
	hipLaunchKernelGGL(k_text_ug_count, dim3(grid_for(U, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, s.u_n, s.u_len, U, with_seq ? MA_TEXT_SEQ_CHUNK : 0u, P<uint32_t>(t->ug_cnt), ctr);
	CHK(scan_exclusive_u32(c, P<uint32_t>(t->ug_cnt), P<uint32_t>(t->ug_rbase), U, nullptr));
	const uint32_t *d_moff = s.moff;
	if (!d_moff) { CHK(scan_exclusive_u32(c, s.u_n, P<uint32_t>(t->ug_moff), U, nullptr)); d_moff = P<uint32_t>(t->ug_moff); }
	CHK(text_ug_member_scan(c, s.mem, M, P<uint32_t>(t->ug_low), P<uint32_t>(t->ug_mscan)));
	if (with_seq && s.arena_bytes) // (asm.c:84 prints the sequence with %s: a NUL byte would end the S line early -- not imitated, the host road takes such an arena)
		hipLaunchKernelGGL(k_text_count_nul, dim3(grid_for(s.arena_bytes / 8 + 1, 256, MA_STREAM_BLOCKS)), dim3(256), 0, c->st, s.arena, s.arena_bytes, ctr);
	HIPCHK(hipGetLastError());
	if (n_links) CHK(xfer_copy(c, t->ug_links.p, (void*)links, (size_t)n_links * 16, 1));
	if (U) CHK(xfer_copy(c, t->ug_ecnt.p, (void*)counts, (size_t)2 * U * 4, 1));
	if (with_seq && !s.plan_uoff) CHK(xfer_copy(c, t->ug_uoff.p, (void*)uoff.data(), ((size_t)U + 1) * 8, 1));
	unsigned long long h_ctr[4] = {0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(h_ctr, t->ctr.p, 32, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	if (h_ctr[3]) return text_host_road(t, info, MAHIP_TEXT_SEQ_NUL, "a NUL byte in the unitig arena");
	const uint64_t n = h_ctr[2] + n_links + U;
	if (n > 0xffffffffull) return text_host_road(t, info, MAHIP_TEXT_TOO_MANY, "the records of the unitig GFA do not fit 32 bits");
	tc_ug_t &g = t->in.ug;
	g.U = U; g.n_links = n_links; g.chunk = MA_TEXT_SEQ_CHUNK; g.n_unit_rec = h_ctr[2];
	g.u_n = s.u_n; g.u_len = s.u_len; g.u_start = s.u_start; g.u_end = s.u_end; g.moff = d_moff; g.rbase = P<uint32_t>(t->ug_rbase); g.mscan = P<uint32_t>(t->ug_mscan);
	g.links = P<uint32_t>(t->ug_links); g.cnt = P<uint32_t>(t->ug_ecnt); g.mem = s.mem; g.uoff = !with_seq ? nullptr : s.plan_uoff ? s.plan_uoff : (const uint64_t*)t->ug_uoff.p; g.arena = with_seq ? s.arena : nullptr;
	info->laps_ms[1] += (TieLaps::now() - t0) * 1e3;
	return text_plan(c, t, MAHIP_TEXT_UG, nullptr, n, d_sub, slab_req, info);
}

uint32_t graph_nseq(const mahip_ctx *c); // graph.hip

extern "C" int mahip_text_prepare_ug(mahip_ctx_t *c, int have_sub, const asg_arc_t *links, uint32_t n_links, int with_seq, mahip_text_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	TextState *t = text_of(c);
	mahip_text_info_t tmp;
	if (!info) info = &tmp;
	text_info_begin(t, MAHIP_TEXT_UG, info);
	if (!mahip_text_enabled()) return text_host_road(t, info, MAHIP_TEXT_SWITCHED_OFF, "MA_TEXT_DEVICE is not 1");
	UgDevView v;
	if (!ug_dev_view(c, &v)) return text_host_road(t, info, MAHIP_TEXT_NO_UG, "the context holds no unitigs");
	const uint32_t Rn = graph_nseq(c);
	if (!t->names || t->n_seq != Rn) return text_host_road(t, info, MAHIP_TEXT_NO_NAMES, "the names on the device do not describe these reads");
	const double t0 = TieLaps::now();
	const uint32_t *d_sub = nullptr;
	if (have_sub) {
		const int rc = text_sub_export(c, t, Rn, &d_sub);
		if (rc < 0) return -1;
		if (rc > 0) return text_host_road(t, info, MAHIP_TEXT_NOMEM, "no device memory for the kept intervals");
	}
	TextUgSrc s = {v.U, v.M, v.u_n, v.u_len, v.u_start, v.u_end, v.u_off, v.mem, nullptr, 0, nullptr, 0};
	if (with_seq) { size_t bytes = 0; if (useq_dev_arena(c, &s.arena, &bytes)) s.arena_bytes = bytes; else s.arena = nullptr; }
	if (with_seq && !useq_plan_uoff(c, v.U, v.M, &s.plan_uoff, &s.plan_tot)) s.plan_uoff = nullptr;
	info->laps_ms[1] = (TieLaps::now() - t0) * 1e3;
	return text_plan_ug(c, t, s, links, n_links, nullptr, d_sub, with_seq, 0, info);
}

extern "C" int mahip_text_emit(mahip_ctx_t *c, mahip_text_sink_t sink, void *arg, mahip_text_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	TextState *t = text_of(c);
	if (!t->planned) { mahip_set_error("mahip_text_emit: nothing prepared"); return -1; }
	t->planned = false;
	double kernel_ms = 0, out_ms = 0;
	int rc = 0, prev_b = -1;
	uint64_t prev_s = 0;
	uint64_t k = 0; // slabs with text so far: they alternate between the two buffers
	for (uint64_t s = 0; s < t->n_slabs && rc == 0; ++s) {
		const uint32_t tot = t->tot_h[s];
		if (tot == 0) continue;
		const int b = (int)(k++ & 1);
		const uint64_t r0 = s * t->slab;
		const uint32_t cnt = (uint32_t)(t->n - r0 < t->slab ? t->n - r0 : t->slab);
		HIPCHK(hipEventRecord(t->ev[b][0], c->st));
		hipLaunchKernelGGL(k_text_write, dim3(grid_for(cnt, 64)), dim3(64), 0, c->st, t->in, r0, cnt, (const uint32_t*)(P<uint32_t>(t->start) + s * t->stride), (char*)t->txt[b].p, P<unsigned long long>(t->ctr));
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(t->ev[b][1], c->st));
		const double t0 = TieLaps::now();
		if (prev_b >= 0) rc = sink(arg, t->host[prev_b], (size_t)t->tot_h[prev_s]); // the slab before goes out while this one is formatted
		if (rc == 0 && xfer_copy(c, t->txt[b].p, t->host[b], tot, 0) != 0) return -1;
		out_ms += (TieLaps::now() - t0) * 1e3;
		float ms = 0;
		if (hipEventElapsedTime(&ms, t->ev[b][0], t->ev[b][1]) == hipSuccess) kernel_ms += ms;
		prev_s = s; prev_b = b;
	}
	if (rc == 0 && prev_b >= 0) {
		const double t0 = TieLaps::now();
		rc = sink(arg, t->host[prev_b], (size_t)t->tot_h[prev_s]);
		out_ms += (TieLaps::now() - t0) * 1e3;
	}
	unsigned long long h_ctr[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(h_ctr, t->ctr.p, 16, hipMemcpyDeviceToHost, c->st));
	HIPCHK(hipStreamSynchronize(c->st));
	t->last.n_slow_lines = h_ctr[1];
	t->last.laps_ms[2] += kernel_ms; t->last.laps_ms[3] = out_ms;
	if (info) *info = t->last;
	if (rc != 0) mahip_set_error("mahip_text_emit: the sink refused the text (%d)", rc);
	return rc;
}

extern "C" int mahip_text_dump(mahip_ctx_t *c, int kind, int have_sub, mahip_text_sink_t sink, void *arg, mahip_text_info_t *info)
{
	mahip_text_info_t tmp;
	if (!info) info = &tmp;
	CHK(mahip_text_prepare(c, kind, have_sub, info));
	if (info->road != MAHIP_TEXT_ROAD_DEVICE) return 0;
	return mahip_text_emit(c, sink, arg, info);
}

extern "C" int mahip_text_last(mahip_ctx_t *c, mahip_text_info_t *info)
{
	*info = text_of(c)->last;
	return 0;
}

struct TextMemSink { char *p; size_t n, cap; };
static int text_mem_sink(void *arg, const char *text, size_t n)
{
	TextMemSink *m = (TextMemSink*)arg;
	if (m->n + n > m->cap) {
		const size_t cap = (m->n + n) * 2 + 4096;
		char *p = (char*)realloc(m->p, cap);
		if (!p) return -1;
		m->p = p; m->cap = cap;
	}
	memcpy(m->p + m->n, text, n);
	m->n += n;
	return 0;
}

extern "C" int mahip_text_format_mem(mahip_ctx_t *c, int kind, const void *records, uint64_t n_records, const void *sub, uint32_t n_seq, const uint8_t *del,
                                     const char *blob, const uint64_t *off, uint64_t slab, char **text, size_t *len, mahip_text_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	if (kind != MAHIP_TEXT_PAF && kind != MAHIP_TEXT_SG && kind != MAHIP_TEXT_BED) { mahip_set_error("mahip_text_format_mem: unknown kind %d", kind); return -1; }
	if ((kind != MAHIP_TEXT_SG && !sub) || (kind == MAHIP_TEXT_BED && n_records != n_seq)) { mahip_set_error("mahip_text_format_mem: a paf or bed dump needs kept intervals, a bed dump one record per read"); return -1; }
	CHK(mahip_text_names(c, blob, off, n_seq, del));
	TextState *t = text_of(c);
	mahip_text_info_t tmp;
	if (!info) info = &tmp;
	text_info_begin(t, kind, info);
	const size_t rec_bytes = kind == MAHIP_TEXT_PAF ? 32 : kind == MAHIP_TEXT_SG ? 16 : 0;
	const double t0 = TieLaps::now();
	CHK(dev_reserve(c, t->rec, n_records * rec_bytes + 16));
	if (n_records * rec_bytes) CHK(xfer_copy(c, t->rec.p, (void*)records, n_records * rec_bytes, 1));
	if (sub) {
		CHK(dev_reserve(c, t->sub, ((size_t)n_seq + 2) * 8));
		if (n_seq) CHK(xfer_copy(c, t->sub.p, (void*)sub, (size_t)n_seq * 8, 1));
	}
	info->laps_ms[1] = (TieLaps::now() - t0) * 1e3;
	CHK(text_plan(c, t, kind, P<uint32_t>(t->rec), n_records, sub ? P<uint32_t>(t->sub) : nullptr, slab, info));
	if (info->road != MAHIP_TEXT_ROAD_DEVICE) { mahip_set_error("mahip_text_format_mem: no memory for the text buffers"); return -1; }
	TextMemSink m = {(char*)malloc(1), 0, 1};
	if (!m.p) { mahip_set_error("mahip_text_format_mem: out of host memory"); return -1; }
	const int rc = mahip_text_emit(c, text_mem_sink, &m, info);
	if (rc != 0) { free(m.p); return -1; }
	*text = m.p; *len = m.n;
	return 0;
}

extern "C" int mahip_text_format_ug_mem(mahip_ctx_t *c, uint32_t n_utg, const uint32_t *u_n, const uint32_t *u_len, const uint32_t *u_start, const uint32_t *u_end, const uint64_t *members,
                                        const asg_arc_t *links, uint32_t n_links, const uint32_t *counts, const void *sub, uint32_t n_seq, int with_seq, const char *arena, uint64_t arena_bytes,
                                        const char *blob, const uint64_t *off, uint64_t slab, char **text, size_t *len, mahip_text_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	CHK(mahip_text_names(c, blob, off, n_seq, nullptr));
	TextState *t = text_of(c);
	mahip_text_info_t tmp;
	if (!info) info = &tmp;
	text_info_begin(t, MAHIP_TEXT_UG, info);
	*text = nullptr; *len = 0;
	const double t0 = TieLaps::now();
	uint64_t M = 0;
	for (uint32_t i = 0; i < n_utg; ++i) M += u_n[i];
	if (M > 0xffffffffull) { mahip_set_error("mahip_text_format_ug_mem: the members do not fit 32 bits"); return -1; }
	struct { DevBuf *b; const void *src; size_t bytes; } up[] = {
		{&t->ug_un, u_n, (size_t)n_utg * 4}, {&t->ug_ulen, u_len, (size_t)n_utg * 4}, {&t->ug_ustart, u_start, (size_t)n_utg * 4}, {&t->ug_uend, u_end, (size_t)n_utg * 4},
		{&t->ug_mem, members, (size_t)M * 8}, {&t->ug_arena, arena, arena ? (size_t)arena_bytes : 0}, {&t->sub, sub, sub ? (size_t)n_seq * 8 : 0}};
	for (auto &u : up) {
		CHK(dev_reserve(c, *u.b, u.bytes + 16));
		if (u.bytes) CHK(xfer_copy(c, u.b->p, (void*)u.src, u.bytes, 1));
	}
	info->laps_ms[1] = (TieLaps::now() - t0) * 1e3;
	TextUgSrc s = {n_utg, (uint32_t)M, P<uint32_t>(t->ug_un), P<uint32_t>(t->ug_ulen), P<uint32_t>(t->ug_ustart), P<uint32_t>(t->ug_uend), nullptr, (const uint64_t*)t->ug_mem.p,
	               arena ? (const char*)t->ug_arena.p : nullptr, arena ? arena_bytes : 0, nullptr, 0};
	CHK(text_plan_ug(c, t, s, links, n_links, counts, sub ? P<uint32_t>(t->sub) : nullptr, with_seq, slab, info));
	if (info->road != MAHIP_TEXT_ROAD_DEVICE) return 0; // a refusal: info->reason says why, there is no text
	TextMemSink m = {(char*)malloc(1), 0, 1};
	if (!m.p) { mahip_set_error("mahip_text_format_ug_mem: out of host memory"); return -1; }
	const int rc = mahip_text_emit(c, text_mem_sink, &m, info);
	if (rc != 0) { free(m.p); return -1; }
	*text = m.p; *len = m.n;
	return 0;
}
