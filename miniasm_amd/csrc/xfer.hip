// xfer.hip -- host<->device bulk copies of pageable memory at PCIe speed.
// hipMemcpy from pageable memory is staged by ONE runtime thread through a pinned bounce buffer (measured
// 3.9 GB/s on the MI355X host); here W worker threads each own two pinned 4 MiB slots: a worker memcpy()s (or
// pread()s) its slices into a slot and queues the DMA on the context's stream, so the CPU copies of all workers
// and the DMA overlap.  No extra streams: creating one costs 8 ms (155 ms for the first of a process) and a
// single stream already moves 57 GB/s (measured, tools/probes/pin_probe.hip).
// Used for the hit records (640 MB per 10 M overlaps), PAF text and the exact-tie key/permutation traffic.
#include "mahip_internal.hpp"
#include <pthread.h>
#include <unistd.h>
#include <sys/stat.h>
#include <time.h>

#define XF_SLOT (4u << 20)
#define XF_MAX_WORKERS 16

struct XferPool {
	int n = 0;
	char *slot[XF_MAX_WORKERS][2] = {};
	bool ready[XF_MAX_WORKERS] = {};
	hipEvent_t ev[XF_MAX_WORKERS][2] = {};
};

struct XferJob { XferPool *p; hipStream_t st; int w, n_workers, dev, to_device, rc, fd; char *dev_ptr; char *host_ptr; size_t bytes, fd_off; }; // fd >= 0: the source is a file (pread)

static void *xfer_worker(void *arg)
{
	XferJob *j = (XferJob*)arg;
	XferPool *p = j->p;
	const int w = j->w;
	if (hipSetDevice(j->dev) != hipSuccess) { j->rc = -1; return 0; }
	if (!p->ready[w]) { // first use of this worker: pin its slots here, in parallel with the other workers
		for (int b = 0; b < 2; ++b) {
			if (hipHostMalloc((void**)&p->slot[w][b], XF_SLOT, hipHostMallocDefault) != hipSuccess) { j->rc = -1; return 0; }
			if (hipEventCreateWithFlags(&p->ev[w][b], hipEventDisableTiming) != hipSuccess) { j->rc = -1; return 0; }
		}
		p->ready[w] = true;
	}
	const hipStream_t st = j->st;
	const size_t n_slices = (j->bytes + XF_SLOT - 1) / XF_SLOT;
	int k = 0;
	for (size_t s = (size_t)w; s < n_slices; s += (size_t)j->n_workers, ++k) {
		const size_t off = s * XF_SLOT, len = j->bytes - off < XF_SLOT ? j->bytes - off : XF_SLOT;
		const int b = k & 1;
		if (j->to_device) {
			if (k >= 2 && hipEventSynchronize(p->ev[w][b]) != hipSuccess) { j->rc = -1; return 0; }
			if (j->fd >= 0) { // file -> pinned slot directly: no pageable intermediate copy
				size_t got = 0;
				while (got < len) {
					ssize_t r = pread(j->fd, p->slot[w][b] + got, len - got, (off_t)(j->fd_off + off + got));
					if (r <= 0) { j->rc = -1; return 0; }
					got += (size_t)r;
				}
			} else memcpy(p->slot[w][b], j->host_ptr + off, len);
			if (hipMemcpyAsync(j->dev_ptr + off, p->slot[w][b], len, hipMemcpyHostToDevice, st) != hipSuccess) { j->rc = -1; return 0; }
			if (hipEventRecord(p->ev[w][b], st) != hipSuccess) { j->rc = -1; return 0; }
		} else { // device -> host: DMA of slice k+1 overlaps the memcpy of slice k
			if (k == 0) {
				if (hipMemcpyAsync(p->slot[w][0], j->dev_ptr + off, len, hipMemcpyDeviceToHost, st) != hipSuccess) { j->rc = -1; return 0; }
				if (hipEventRecord(p->ev[w][0], st) != hipSuccess) { j->rc = -1; return 0; }
			}
			const size_t s2 = s + (size_t)j->n_workers;
			if (s2 < n_slices) {
				const size_t off2 = s2 * XF_SLOT, len2 = j->bytes - off2 < XF_SLOT ? j->bytes - off2 : XF_SLOT;
				if (hipMemcpyAsync(p->slot[w][b ^ 1], j->dev_ptr + off2, len2, hipMemcpyDeviceToHost, st) != hipSuccess) { j->rc = -1; return 0; }
				if (hipEventRecord(p->ev[w][b ^ 1], st) != hipSuccess) { j->rc = -1; return 0; }
			}
			if (hipEventSynchronize(p->ev[w][b]) != hipSuccess) { j->rc = -1; return 0; }
			memcpy(j->host_ptr + off, p->slot[w][b], len);
		}
	}
	if (hipStreamSynchronize(st) != hipSuccess) j->rc = -1;
	return 0;
}

extern "C" int ma_cpu_budget(void);
static int xfer_workers(int to_device)
{
	const char *s = getenv("MA_XFER_THREADS");
	long n = s ? atol(s) : ma_cpu_budget(); // (the control group's CPU quota counts, not the machine's core count: host/ingest_mt.c)
	// device -> host ends in a memcpy into pageable memory that is usually fresh (a page fault and a cleared page per 4 KB): 8 workers reach 21 GB/s, 16 reach 31
	// (8 GB of tie-walk keys, BASELINE configs[4], profiles/r03_tiewalk.txt); host -> device is at 45 GB/s with 8 and no faster with 16
	const long most = to_device ? 8 : 16;
	if (n < 1) n = 1;
	if (n > most && !s) n = most;
	if (n > XF_MAX_WORKERS) n = XF_MAX_WORKERS;
	return (int)n;
}

static int xfer_pool_init(mahip_ctx *c, int n)
{
	if (!c->xfer) c->xfer = new XferPool();
	XferPool *p = (XferPool*)c->xfer;
	if (p->n < n) p->n = n; // slots, events and the stream of a worker are created by the worker on first use
	return 0;
}

void xfer_pool_free(mahip_ctx *c)
{
	XferPool *p = (XferPool*)c->xfer;
	if (!p) return;
	for (int w = 0; w < p->n; ++w) {
		for (int b = 0; b < 2; ++b) { if (p->slot[w][b]) (void)hipHostFree(p->slot[w][b]); if (p->ev[w][b]) (void)hipEventDestroy(p->ev[w][b]); }
	}
	delete p;
	c->xfer = nullptr;
}

// synchronous with respect to the host; ordered after everything already queued on the context's stream
static int xfer_run(mahip_ctx *c, void *dev_ptr, void *host_ptr, int fd, size_t bytes, int to_device, size_t fd_off = 0)
{
	if (bytes == 0) return 0;
	HIPCHK(hipSetDevice(c->dev));
	if (fd < 0 && bytes < (8u << 20)) { // small: the runtime's own path
		c->xfer_last = { MAHIP_XFER_RUNTIME, to_device, (uint64_t)bytes, 0, 0 };
		HIPCHK(hipMemcpyAsync(to_device ? dev_ptr : host_ptr, to_device ? host_ptr : dev_ptr, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->st));
		HIPCHK(hipStreamSynchronize(c->st));
		return 0;
	}
	int W = xfer_workers(to_device);
	const size_t n_slices = (bytes + XF_SLOT - 1) / XF_SLOT;
	if ((size_t)W > n_slices) W = (int)n_slices;
	c->xfer_last = { fd >= 0 ? MAHIP_XFER_STAGED_FILE : MAHIP_XFER_STAGED_MEM, to_device, (uint64_t)bytes, (uint64_t)n_slices, W };
	CHK(xfer_pool_init(c, W));
	XferJob job[XF_MAX_WORKERS];
	pthread_t th[XF_MAX_WORKERS];
	bool started[XF_MAX_WORKERS];
	for (int w = 0; w < W; ++w) {
		job[w].p = (XferPool*)c->xfer; job[w].st = c->st; job[w].w = w; job[w].n_workers = W; job[w].dev = c->dev; job[w].to_device = to_device; job[w].rc = 0;
		job[w].dev_ptr = (char*)dev_ptr; job[w].host_ptr = (char*)host_ptr; job[w].bytes = bytes; job[w].fd = fd; job[w].fd_off = fd_off;
		started[w] = pthread_create(&th[w], 0, xfer_worker, &job[w]) == 0;
		if (!started[w]) xfer_worker(&job[w]); // no thread: do this worker's slices here
	}
	int rc = 0;
	const bool timing = ma_timing_level() >= 1;
	struct timespec ts0, ts1;
	if (timing) clock_gettime(CLOCK_MONOTONIC, &ts0);
	for (int w = 0; w < W; ++w) {
		if (started[w]) pthread_join(th[w], 0);
		if (job[w].rc != 0) rc = -1;
	}
	if (timing) {
		clock_gettime(CLOCK_MONOTONIC, &ts1);
		double dt = (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec);
		fprintf(stderr, "[T::xfer] %s %.0f MB, %d workers: %.3f s (%.1f GB/s)\n", fd >= 0 ? "file->HBM" : to_device ? "host->HBM" : "HBM->host", (double)bytes / 1e6, W, dt, (double)bytes / dt / 1e9);
	}
	if (rc) {
		mahip_set_error("xfer_copy: staged copy failed (%s)", hipGetErrorString(hipGetLastError()));
		// a worker that failed returned without its final wait, and the others may have waited before it queued its last DMA: that DMA may still be reading a
		// pinned slot, which the next copy's first two slices per worker refill without looking at the slot's event
		(void)hipStreamSynchronize(c->st);
		return -1;
	}
	return 0;
}

int xfer_copy(mahip_ctx *c, void *dev_ptr, void *host_ptr, size_t bytes, int to_device) { return xfer_run(c, dev_ptr, host_ptr, -1, bytes, to_device); }
// bytes [0, bytes) of an open file -> device memory
int xfer_from_fd(mahip_ctx *c, void *dev_ptr, int fd, size_t bytes) { return xfer_run(c, dev_ptr, nullptr, fd, bytes, 1); }
// bytes [off, off + bytes) of an open file -> device memory (a rank's own range of the text: host/ingest_sharded.c)
int xfer_from_fd_at(mahip_ctx *c, void *dev_ptr, int fd, size_t off, size_t bytes) { return xfer_run(c, dev_ptr, nullptr, fd, bytes, 1, off); }

extern "C" int mahip_memcpy_h2d(mahip_ctx_t *c, void *d_dst, const void *h_src, size_t bytes) { return xfer_copy(c, d_dst, (void*)h_src, bytes, 1); }
extern "C" int mahip_memcpy_d2h(mahip_ctx_t *c, void *h_dst, const void *d_src, size_t bytes) { return xfer_copy(c, (void*)d_src, h_dst, bytes, 0); }
extern "C" int mahip_memcpy_fd2d(mahip_ctx_t *c, void *d_dst, int fd, size_t off, size_t nbytes) { return xfer_from_fd_at(c, d_dst, fd, off, nbytes); } // for stage tests
extern "C" int mahip_xfer_last(mahip_ctx_t *c, mahip_xfer_info_t *out) { *out = c->xfer_last; return 0; }                                                // for stage tests

// ================================================================================================ bgzip-compressed input, inflated on the device
// A BGZF file goes to HBM as it is (xfer_from_fd), the host's block table follows (host/ingest_gpu.c: ma_bgzf_walk), ONE WAVE inflates ONE member into its
// slice of the text buffer (inflate_core.h) and a second pass checks every member's CRC-32 over the finished text.  The text buffer is the PAF reader's or
// the reads-file reader's own, so their kernels take over unchanged.  Output offsets and the text size are 64-bit throughout (the table's out_off, the
// pointer arithmetic of both kernels, the reservation): the text of a big overlap file exceeds 4 GiB; what is 32-bit is per member (<= 64 KiB either way).
#include "inflate_core.h"

#define BGZF_WAVES 4u // members per workgroup: 4 x sizeof(InfLds) = 148 KiB of the CU's 160 KiB
enum { BG_RES_BAD = 0, BG_RES_STORED, BG_RES_FIXED, BG_RES_DYNAMIC, BG_RES_WORDS = 8 }; // res[BG_RES_BAD] = min over the members with a status of member << 8 | status

__global__ __launch_bounds__(256) void k_bgzf_inflate(const uint8_t *__restrict__ comp, const mahip_bgzf_member_t *__restrict__ tab, uint64_t n_members, uint8_t *__restrict__ text,
                                                      unsigned long long *__restrict__ res)
{
	__shared__ InfLds s_lds[BGZF_WAVES];
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t m = (uint64_t)blockIdx.x * BGZF_WAVES + wave;
	if (m >= n_members) return; // the whole wave; nothing below waits for another wave
	const mahip_bgzf_member_t mb = tab[m];
	uint32_t nblk[3];
	const uint32_t st = inf_member(comp + mb.in_off, mb.in_len, text + mb.out_off, mb.isize, s_lds[wave], lane, nblk);
	if (lane == 0) {
		if (st) atomicMin(res + BG_RES_BAD, (unsigned long long)(m << 8 | st));
		if (nblk[0]) atomicAdd(res + BG_RES_STORED, (unsigned long long)nblk[0]);
		if (nblk[1]) atomicAdd(res + BG_RES_FIXED, (unsigned long long)nblk[1]);
		if (nblk[2]) atomicAdd(res + BG_RES_DYNAMIC, (unsigned long long)nblk[2]);
	}
}

// one wave per member: lane i runs the table-driven CRC over the i-th 64th of the member's text, the lanes' values are moved in front of the bytes that follow
// them (times x^(8 n) mod P) and XORed together
__global__ __launch_bounds__(256) void k_bgzf_crc(const uint8_t *__restrict__ text, const mahip_bgzf_member_t *__restrict__ tab, uint64_t n_members, unsigned long long *__restrict__ res)
{
	__shared__ uint32_t s_crc[256];
	{
		uint32_t v = threadIdx.x;
		for (int k = 0; k < 8; ++k) v = v & 1u ? (v >> 1) ^ INF_CRC_POLY : v >> 1;
		s_crc[threadIdx.x] = v;
	}
	__syncthreads();
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t m = (uint64_t)blockIdx.x * BGZF_WAVES + wave;
	if (m >= n_members) return;
	const mahip_bgzf_member_t mb = tab[m];
	const uint8_t *t = text + mb.out_off;
	const uint32_t piece = (mb.isize + 63u) / 64u;
	const uint32_t b = lane * piece < mb.isize ? lane * piece : mb.isize, e = b + piece < mb.isize ? b + piece : mb.isize;
	uint32_t crc = 0xffffffffu;
	for (uint32_t p = b; p < e; ++p) crc = s_crc[(crc ^ t[p]) & 255u] ^ (crc >> 8);
	crc = ~crc; // (an empty piece: 0)
	crc = inf_mulmod(crc, inf_xpow8(mb.isize - e));
	for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
	if (lane == 0 && crc != mb.crc) atomicMin(res + BG_RES_BAD, (unsigned long long)(m << 8 | INF_CRC));
}

extern "C" int ma_bgzf_walk(int fd, const void *mem, uint64_t nbytes, mahip_bgzf_member_t **tab, uint64_t *n_members, uint64_t *n_empty, uint64_t *text_bytes, int64_t *bad);

static double bg_now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + ts.tv_nsec * 1e-9; }

// the context remembers what a load decided; MA_PIPE_TIMING prints it
static void bgzf_report(mahip_ctx *c, const mahip_bgzf_info_t *info)
{
	c->bgzf_last = *info;
	if (ma_timing_level() < 1) return;
	if (info->reason == MAHIP_BGZF_OK)
		fprintf(stderr, "[T::bgzf] reader=device members=%llu (%llu empty) %.1f MB -> %.1f MB: walk %.3f upload %.3f inflate %.3f crc %.3f ms (inflate %.2f GB/s of text)\n", (unsigned long long)info->n_members,
		        (unsigned long long)info->n_empty, (double)info->comp_bytes / 1e6, (double)info->text_bytes / 1e6, info->laps_ms[0], info->laps_ms[1], info->laps_ms[2], info->laps_ms[3],
		        info->laps_ms[2] > 0 ? (double)info->text_bytes / info->laps_ms[2] / 1e6 : 0.0);
	else fprintf(stderr, "[T::bgzf] reader=host reason=%d (%s) member=%lld\n", info->reason, mahip_bgzf_reason_name(info->reason), (long long)info->first_bad_member);
}

// fd >= 0: an open regular file of nbytes; else an image in host memory.  target 0: the text goes to `out` (host, out_cap bytes) and nothing stays loaded.
static int bgzf_run(mahip_ctx *c, int fd, const void *mem, size_t nbytes, int target, void *out, size_t out_cap, mahip_bgzf_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	memset(info, 0, sizeof(*info));
	info->reader = MAHIP_BGZF_HOST; info->first_bad_member = -1; info->comp_bytes = nbytes;
	mahip_bgzf_member_t *tab = nullptr;
	uint64_t n = 0;
	double t0 = bg_now(), t1;
	const int wr = ma_bgzf_walk(fd, mem, nbytes, &tab, &n, &info->n_empty, &info->text_bytes, &info->first_bad_member);
	if (wr < 0) { mahip_set_error("mahip_bgzf_load: cannot read the compressed input"); return -1; }
	info->laps_ms[0] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
	info->reason = wr; info->n_members = n;
	if (wr != MAHIP_BGZF_OK) { bgzf_report(c, info); return 0; }
	const uint64_t text_bytes = info->text_bytes;
	DevBuf d_comp, d_tab, d_res, d_own;
	void *d_text = nullptr;
	int rc = 0;
	// the text first, the way the reader it is for reserves it (the PAF reader's cap, MA_PAF_MAX_BYTES, counts the inflated bytes)
	if (target == MAHIP_BGZF_PAF) { if (paf_text_reserve(c, (size_t)text_bytes, &d_text) != 0) { free(tab); return -1; } }
	else if (target == MAHIP_BGZF_FASTX) {
		if (text_bytes == 0) info->reason = MAHIP_BGZF_EMPTY;
		else if (fx_text_reserve(c, (size_t)text_bytes, &d_text) != 0) info->reason = MAHIP_BGZF_NOMEM;
	} else {
		if (out_cap < text_bytes) { free(tab); mahip_set_error("mahip_bgzf_inflate_mem: %llu bytes of text, room for %zu", (unsigned long long)text_bytes, out_cap); return -1; }
		if (dev_reserve(c, d_own, (size_t)text_bytes + 64) != 0) info->reason = MAHIP_BGZF_NOMEM;
		d_text = d_own.p;
	}
	if (info->reason == MAHIP_BGZF_OK && (dev_reserve(c, d_comp, nbytes + 64) != 0 || dev_reserve(c, d_tab, (size_t)n * sizeof(mahip_bgzf_member_t)) != 0 || dev_reserve(c, d_res, BG_RES_WORDS * 8) != 0))
		info->reason = MAHIP_BGZF_NOMEM;
	if (info->reason == MAHIP_BGZF_OK) {
		unsigned long long h_res[BG_RES_WORDS];
		const unsigned grid = (unsigned)((n + BGZF_WAVES - 1) / BGZF_WAVES);
		do { // (one pass; `break` = a real error)
			rc = -1;
			if ((fd >= 0 ? xfer_from_fd(c, d_comp.p, fd, nbytes) : xfer_copy(c, d_comp.p, (void*)mem, nbytes, 1)) != 0) break;
			if (hipMemcpyAsync(d_tab.p, tab, (size_t)n * sizeof(mahip_bgzf_member_t), hipMemcpyHostToDevice, c->st) != hipSuccess) break;
			if (hipMemsetAsync(d_res.p, 0, BG_RES_WORDS * 8, c->st) != hipSuccess || hipMemsetAsync(d_res.p, 0xff, 8, c->st) != hipSuccess) break;
			if (hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[1] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
			{
				ProfScope ps(c, "k_bgzf_inflate", (double)nbytes + (double)text_bytes);
				hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(256), 0, c->st, (const uint8_t*)d_comp.p, (const mahip_bgzf_member_t*)d_tab.p, n, (uint8_t*)d_text, P<unsigned long long>(d_res));
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[2] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
			{
				ProfScope ps(c, "k_bgzf_crc", (double)text_bytes);
				hipLaunchKernelGGL(k_bgzf_crc, dim3(grid), dim3(256), 0, c->st, (const uint8_t*)d_text, (const mahip_bgzf_member_t*)d_tab.p, n, P<unsigned long long>(d_res));
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipMemcpyAsync(h_res, d_res.p, BG_RES_WORDS * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[3] = (bg_now() - t0) * 1e3;
			rc = 0;
			info->n_stored = h_res[BG_RES_STORED]; info->n_fixed = h_res[BG_RES_FIXED]; info->n_dynamic = h_res[BG_RES_DYNAMIC];
			if (h_res[BG_RES_BAD] != ~0ull) {
				info->reason = MAHIP_BGZF_BAD_BTYPE + (int)(h_res[BG_RES_BAD] & 255u) - 1;
				info->first_bad_member = (int64_t)(h_res[BG_RES_BAD] >> 8);
			} else if (target == 0 && text_bytes) rc = xfer_copy(c, d_text, out, (size_t)text_bytes, 0);
		} while (0);
		if (rc != 0) mahip_set_error("mahip_bgzf_load: upload, launch or copy failed (%s)", hipGetErrorString(hipGetLastError()));
	}
	(void)hipStreamSynchronize(c->st);
	dev_free(c, d_comp); dev_free(c, d_tab); dev_free(c, d_res); dev_free(c, d_own);
	free(tab);
	if (rc == 0 && info->reason == MAHIP_BGZF_OK) {
		info->reader = MAHIP_BGZF_DEVICE;
		if (target == MAHIP_BGZF_PAF) paf_text_loaded(c); else if (target == MAHIP_BGZF_FASTX) fx_text_loaded(c);
	} else { // nothing stays loaded: the caller inflates with zlib
		if (target == MAHIP_BGZF_PAF) (void)mahip_paf_release(c); else if (target == MAHIP_BGZF_FASTX) (void)mahip_fastx_release(c);
	}
	if (rc == 0) bgzf_report(c, info); else c->bgzf_last = *info;
	return rc;
}

extern "C" int mahip_bgzf_load_fd(mahip_ctx_t *c, int fd, size_t nbytes, int target, mahip_bgzf_info_t *info)
{
	if (target != MAHIP_BGZF_PAF && target != MAHIP_BGZF_FASTX) { mahip_set_error("mahip_bgzf_load_fd: target %d", target); return -1; }
	return bgzf_run(c, fd, nullptr, nbytes, target, nullptr, 0, info);
}
extern "C" int mahip_bgzf_load_mem(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, mahip_bgzf_info_t *info)
{
	if (target != MAHIP_BGZF_PAF && target != MAHIP_BGZF_FASTX) { mahip_set_error("mahip_bgzf_load_mem: target %d", target); return -1; }
	return bgzf_run(c, -1, comp, nbytes, target, nullptr, 0, info);
}
extern "C" int mahip_bgzf_inflate_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, void *out, size_t out_cap, mahip_bgzf_info_t *info) { return bgzf_run(c, -1, comp, ncomp, 0, out, out_cap, info); }

// ---- a rank's own range of a BGZF overlap file (include/mahip.h: mahip_bgzf_load_fd_range)
// bit 7 of every byte of w that is '\n' (useq.hip: fx_eq)
__device__ __forceinline__ uint32_t tx_nl(uint32_t w) { const uint32_t x = w ^ 0x0a0a0a0au; return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

#define TX_WAVE_BYTES 1024u // 64 lanes x 16 bytes: what a wave looks at in one step

// *res (preset to all ones) = min(*res, position of the first '\n' among t[from .. to)).  The bytes between the first and the last 16-byte boundary of the
// ADDRESS range are read as 16-byte words, a wave taking TX_WAVE_BYTES consecutive ones a step; waves go up through the text, so a wave's first step with a
// newline holds its smallest one, and a wave stops as soon as *res lies in front of it.  BOUNDS: words are read at a0 <= w, w + 16 <= a1 with from <= a0 and
// a1 <= to; the fewer than 16 bytes in front of a0 and behind a1 are read one by one, by block 0.
__global__ __launch_bounds__(256) void k_text_first_nl(const uint8_t *__restrict__ t, uint64_t from, uint64_t to, unsigned long long *res)
{
	const uint64_t mis = (uint64_t)(uintptr_t)(t + from) & 15u;
	uint64_t a0 = from + (mis ? 16u - mis : 0u);
	if (a0 > to) a0 = to;
	const uint64_t a1 = a0 + ((to - a0) & ~(uint64_t)15);
	if (blockIdx.x == 0 && threadIdx.x < 32) { // [from, a0) and [a1, to)
		const unsigned k = threadIdx.x & 15u;
		const uint64_t p = (threadIdx.x < 16 ? from : a1) + k, lim = threadIdx.x < 16 ? a0 : to;
		if (p < lim && t[p] == '\n') atomicMin(res, (unsigned long long)p);
	}
	const unsigned lane = threadIdx.x & 63;
	const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4u;
	uint64_t best = ~0ull;
	for (uint64_t base = a0 + wave * TX_WAVE_BYTES; base < a1; base += n_waves * TX_WAVE_BYTES) { // the whole wave
		if (wv_ballot(*(volatile const unsigned long long*)res < base)) break; // the whole wave, whichever lane saw it (a stale value only costs steps)
		const uint64_t w = base + lane * 16u;
		if (w < a1) {
			const uint4 v = *(const uint4*)(t + w);
			const uint32_t m[4] = {tx_nl(v.x), tx_nl(v.y), tx_nl(v.z), tx_nl(v.w)};
			for (int k = 3; k >= 0; --k) if (m[k]) best = w + 4u * (unsigned)k + ((unsigned)__builtin_ctz(m[k]) >> 3);
		}
		if (wv_ballot(best != ~0ull)) break;
	}
	best = ~wv_max_u64(~best);
	if (lane == 0 && best != ~0ull) atomicMin(res, (unsigned long long)best);
}

// queued: d_word <- all ones, the search.  The caller fetches the word.
static int text_first_nl_launch(mahip_ctx *c, const void *d_text, uint64_t from, uint64_t to, DevBuf &d_word)
{
	HIPCHK(hipMemsetAsync(d_word.p, 0xff, 8, c->st));
	if (to <= from) return 0;
	ProfScope ps(c, "k_text_first_nl", (double)(to - from));
	hipLaunchKernelGGL(k_text_first_nl, dim3(grid_for((size_t)(to - from), 4 * TX_WAVE_BYTES, 1024)), dim3(256), 0, c->st, (const uint8_t*)d_text, from, to, P<unsigned long long>(d_word));
	HIPCHK(hipGetLastError());
	return 0;
}

extern "C" int mahip_text_first_nl(mahip_ctx_t *c, const void *d_text, uint64_t from, uint64_t to, uint64_t *pos)
{
	HIPCHK(hipSetDevice(c->dev));
	DevBuf d_word;
	unsigned long long h = ~0ull;
	CHK(dev_reserve(c, d_word, 64));
	int rc = text_first_nl_launch(c, d_text, from, to, d_word);
	if (rc == 0 && (hipMemcpyAsync(&h, d_word.p, 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)) {
		mahip_set_error("mahip_text_first_nl: %s", hipGetErrorString(hipGetLastError()));
		rc = -1;
	}
	(void)hipStreamSynchronize(c->st);
	dev_free(c, d_word);
	*pos = h;
	return rc;
}

// members [m0, m1) of the chain, inflated into a buffer of their own: bytes [t0, t1) of the inflated file
struct BgBatch { DevBuf text; uint64_t m0, m1, t0, t1; };
struct BgRange { // one mahip_bgzf_load_fd_range / mahip_bgzf_range_mem
	int fd; const uint8_t *mem;
	const mahip_bgzf_member_t *tab; uint64_t n, T;
	std::vector<BgBatch> bs;
	DevBuf d_res; // BG_RES_WORDS words of the two kernels + the word of the search
	mahip_bgzf_range_t *range; mahip_bgzf_info_t *info;
};

// Upload, inflate and CRC-check members [m0, m1), m0 < m1 <= n.  The table rows are rebased on the host: in_off counts from the first member's deflate bytes
// (the upload starts there and ends with the last member's), out_off from the first member's text; both stay 64-bit.  0 with info->reason set (a status, with
// the member's number in the WHOLE chain, or NOMEM), -1: a real error.
static int bgzf_range_batch(mahip_ctx *c, BgRange &r, uint64_t m0, uint64_t m1)
{
	mahip_bgzf_info_t *info = r.info;
	const mahip_bgzf_member_t *tab = r.tab;
	const uint64_t nm = m1 - m0, c0 = tab[m0].in_off, span = tab[m1 - 1].in_off + tab[m1 - 1].in_len - c0, t0 = tab[m0].out_off, t1 = m1 < r.n ? tab[m1].out_off : r.T;
	DevBuf d_comp, d_tab;
	BgBatch b;
	b.m0 = m0; b.m1 = m1; b.t0 = t0; b.t1 = t1;
	mahip_bgzf_member_t *rows = (mahip_bgzf_member_t*)malloc((size_t)nm * sizeof(*rows));
	if (rows == nullptr) { mahip_set_error("mahip_bgzf_load_fd_range: out of host memory"); return -1; }
	for (uint64_t k = 0; k < nm; ++k) { rows[k] = tab[m0 + k]; rows[k].in_off -= c0; rows[k].out_off -= t0; }
	int rc = 0;
	if (dev_reserve(c, b.text, (size_t)(t1 - t0) + 64) != 0 || dev_reserve(c, d_comp, (size_t)span + 64) != 0 || dev_reserve(c, d_tab, (size_t)nm * sizeof(*rows)) != 0) info->reason = MAHIP_BGZF_NOMEM;
	else {
		unsigned long long h_res[BG_RES_WORDS];
		const unsigned grid = (unsigned)((nm + BGZF_WAVES - 1) / BGZF_WAVES);
		double t = bg_now(), u;
		do { // (one pass; `break` = a real error)
			rc = -1;
			if ((r.fd >= 0 ? xfer_from_fd_at(c, d_comp.p, r.fd, (size_t)c0, (size_t)span) : xfer_copy(c, d_comp.p, (void*)(r.mem + c0), (size_t)span, 1)) != 0) break;
			if (hipMemcpyAsync(d_tab.p, rows, (size_t)nm * sizeof(*rows), hipMemcpyHostToDevice, c->st) != hipSuccess) break;
			if (hipMemsetAsync(r.d_res.p, 0, BG_RES_WORDS * 8, c->st) != hipSuccess || hipMemsetAsync(r.d_res.p, 0xff, 8, c->st) != hipSuccess) break;
			if (hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[1] += ((u = bg_now()) - t) * 1e3; t = u;
			{
				ProfScope ps(c, "k_bgzf_inflate", (double)span + (double)(t1 - t0));
				hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(256), 0, c->st, (const uint8_t*)d_comp.p, (const mahip_bgzf_member_t*)d_tab.p, nm, (uint8_t*)b.text.p, P<unsigned long long>(r.d_res));
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[2] += ((u = bg_now()) - t) * 1e3; t = u;
			{
				ProfScope ps(c, "k_bgzf_crc", (double)(t1 - t0));
				hipLaunchKernelGGL(k_bgzf_crc, dim3(grid), dim3(256), 0, c->st, (const uint8_t*)b.text.p, (const mahip_bgzf_member_t*)d_tab.p, nm, P<unsigned long long>(r.d_res));
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipMemcpyAsync(h_res, r.d_res.p, BG_RES_WORDS * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
			info->laps_ms[3] += (bg_now() - t) * 1e3;
			rc = 0;
			info->n_stored += h_res[BG_RES_STORED]; info->n_fixed += h_res[BG_RES_FIXED]; info->n_dynamic += h_res[BG_RES_DYNAMIC];
			if (h_res[BG_RES_BAD] != ~0ull) {
				info->reason = MAHIP_BGZF_BAD_BTYPE + (int)(h_res[BG_RES_BAD] & 255u) - 1;
				info->first_bad_member = (int64_t)(m0 + (h_res[BG_RES_BAD] >> 8));
			}
		} while (0);
		if (rc != 0) mahip_set_error("mahip_bgzf_load_fd_range: upload, launch or copy failed (%s)", hipGetErrorString(hipGetLastError()));
		r.range->comp_bytes_uploaded += span;
	}
	(void)hipStreamSynchronize(c->st);
	dev_free(c, d_comp); dev_free(c, d_tab);
	free(rows);
	r.bs.push_back(b); // (the caller frees the text with the others)
	return rc;
}

// ls(a) for 0 < a < T: the byte behind the first '\n' at a position >= from (from >= a - 1, nothing in [a - 1, from) is one), T when the chain ends without
// one.  Members [.., *hi) are inflated; what the search needs beyond them is inflated here, *batch members and twice as many each further round.
static int bgzf_range_border(mahip_ctx *c, BgRange &r, uint64_t from, uint64_t *hi, uint64_t *batch, uint64_t *ls)
{
	for (;;) {
		for (size_t k = 0; k < r.bs.size(); ++k) {
			const BgBatch &b = r.bs[k];
			if (b.t1 <= from) continue;
			const uint64_t f = from > b.t0 ? from : b.t0;
			unsigned long long h = ~0ull;
			CHK(text_first_nl_launch(c, b.text.p, f - b.t0, b.t1 - b.t0, r.d_res));
			HIPCHK(hipMemcpyAsync(&h, r.d_res.p, 8, hipMemcpyDeviceToHost, c->st));
			HIPCHK(hipStreamSynchronize(c->st));
			if (h != ~0ull) { *ls = b.t0 + h + 1; return 0; }
			from = b.t1;
		}
		if (*hi == r.n) { *ls = r.T; return 0; }
		const uint64_t m1 = r.n - *hi < *batch ? r.n : *hi + *batch;
		CHK(bgzf_range_batch(c, r, *hi, m1));
		*hi = m1; *batch *= 2; ++r.range->n_rounds;
		if (r.info->reason != MAHIP_BGZF_OK) return 0;
	}
}

// fd >= 0: an open regular file of nbytes, the text stays loaded in the PAF reader; else an image in host memory, the text goes to `out` (host, out_cap bytes)
static int bgzf_range_run(mahip_ctx *c, int fd, const void *mem, size_t nbytes, int rank, int world, void *out, size_t out_cap, mahip_bgzf_range_t *range, mahip_bgzf_info_t *info)
{
	HIPCHK(hipSetDevice(c->dev));
	if (world < 1 || rank < 0 || rank >= world) { mahip_set_error("mahip_bgzf_load_fd_range: rank %d of %d", rank, world); return -1; }
	const bool keep = fd >= 0;
	memset(info, 0, sizeof(*info));
	memset(range, 0, sizeof(*range));
	info->reader = MAHIP_BGZF_HOST; info->first_bad_member = -1; info->comp_bytes = nbytes;
	mahip_bgzf_member_t *tab = nullptr;
	uint64_t n = 0;
	const double t0 = bg_now();
	const int wr = ma_bgzf_walk(fd, mem, nbytes, &tab, &n, &info->n_empty, &info->text_bytes, &info->first_bad_member);
	if (wr < 0) { mahip_set_error("mahip_bgzf_load_fd_range: cannot read the compressed input"); return -1; }
	info->laps_ms[0] = (bg_now() - t0) * 1e3;
	info->reason = wr; info->n_members = n;
	if (wr != MAHIP_BGZF_OK) { if (keep) (void)mahip_paf_release(c); c->bgzf_last = *info; return 0; }
	const uint64_t T = info->text_bytes, nom_b = T * (uint64_t)rank / (uint64_t)world, nom_e = rank + 1 == world ? T : T * (uint64_t)(rank + 1) / (uint64_t)world;
	range->text_bytes = T;
	BgRange r;
	r.fd = fd; r.mem = (const uint8_t*)mem; r.tab = tab; r.n = n; r.T = T; r.range = range; r.info = info;
	auto member_of = [&](uint64_t byte) { // the first member whose text ends behind `byte`; n: none
		uint64_t lo = 0, hi = n;
		while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (tab[mid].out_off + tab[mid].isize > byte) hi = mid; else lo = mid + 1; }
		return lo;
	};
	range->first_member = member_of(nom_b ? nom_b - 1 : 0);
	DevBuf d_own;
	void *d_text = nullptr;
	uint64_t beg = 0, end = 0;
	int rc = 0;
	bool said = false; // the error message is set
	do { // (one pass; `break` with rc = -1: a real error; with rc = 0: done, info->reason says how)
		if (nom_e > 0) { // (else: T < world and the rank's nominal range ends at byte 0 -- nothing in front of it to own)
			if (dev_reserve(c, r.d_res, (BG_RES_WORDS + 8) * 8) != 0) { info->reason = MAHIP_BGZF_NOMEM; break; }
			uint64_t hi = member_of(nom_e - 1) + 1 + MAHIP_BGZF_RANGE_AHEAD, batch = MAHIP_BGZF_RANGE_AHEAD;
			if (hi > n) hi = n;
			said = true;
			if ((rc = bgzf_range_batch(c, r, range->first_member, hi)) != 0 || info->reason != MAHIP_BGZF_OK) break;
			if (nom_b > 0 && ((rc = bgzf_range_border(c, r, nom_b - 1, &hi, &batch, &beg)) != 0 || info->reason != MAHIP_BGZF_OK)) break;
			if (nom_e >= T) end = T;
			else if ((rc = bgzf_range_border(c, r, nom_e > beg ? nom_e - 1 : beg - 1, &hi, &batch, &end)) != 0 || info->reason != MAHIP_BGZF_OK) break; // (no newline in [nom_b - 1, beg - 1))
			said = false;
			if (end < beg) end = beg;
			range->n_members_inflated = hi - range->first_member;
		}
		range->beg = beg; range->end = end;
		// the text, the way mahip_paf_load_fd_range reserves it (the PAF reader's cap, MA_PAF_MAX_BYTES, counts the rank's own bytes)
		if (keep) { if (paf_text_reserve(c, (size_t)(end - beg), &d_text) != 0) { rc = -1; said = true; break; } }
		else {
			if (out_cap < end - beg) { mahip_set_error("mahip_bgzf_range_mem: %llu bytes of text, room for %zu", (unsigned long long)(end - beg), out_cap); rc = -1; said = true; break; }
			if (dev_reserve(c, d_own, (size_t)(end - beg) + 64) != 0) { info->reason = MAHIP_BGZF_NOMEM; break; }
			d_text = d_own.p;
		}
		rc = -1;
		bool ok = true;
		for (size_t k = 0; k < r.bs.size() && ok; ++k) { // bytes [beg, end) of the batches -> the text, one copy a batch
			const BgBatch &b = r.bs[k];
			const uint64_t lo = beg > b.t0 ? beg : b.t0, hi = end < b.t1 ? end : b.t1;
			if (lo < hi) ok = hipMemcpyAsync((uint8_t*)d_text + (lo - beg), (const uint8_t*)b.text.p + (lo - b.t0), (size_t)(hi - lo), hipMemcpyDeviceToDevice, c->st) == hipSuccess;
		}
		if (!ok || hipStreamSynchronize(c->st) != hipSuccess) break;
		rc = !keep && end > beg ? xfer_copy(c, d_text, out, (size_t)(end - beg), 0) : 0;
		said = rc != 0;
	} while (0);
	if (rc != 0 && !said) mahip_set_error("mahip_bgzf_load_fd_range: launch or copy failed (%s)", hipGetErrorString(hipGetLastError()));
	(void)hipStreamSynchronize(c->st);
	if (info->reason != MAHIP_BGZF_OK || rc != 0) { range->beg = range->end = 0; range->n_members_inflated = r.bs.empty() ? 0 : r.bs.back().m1 - range->first_member; }
	for (size_t k = 0; k < r.bs.size(); ++k) dev_free(c, r.bs[k].text);
	dev_free(c, r.d_res); dev_free(c, d_own);
	free(tab);
	if (rc == 0 && info->reason == MAHIP_BGZF_OK) {
		info->reader = MAHIP_BGZF_DEVICE;
		if (keep) paf_text_loaded(c);
	} else if (keep) (void)mahip_paf_release(c); // nothing stays loaded
	c->bgzf_last = *info;
	return rc;
}

extern "C" int mahip_bgzf_load_fd_range(mahip_ctx_t *c, int fd, size_t nbytes, int rank, int world, mahip_bgzf_range_t *range, mahip_bgzf_info_t *info)
{
	if (fd < 0) { mahip_set_error("mahip_bgzf_load_fd_range: no file"); return -1; }
	return bgzf_range_run(c, fd, nullptr, nbytes, rank, world, nullptr, 0, range, info);
}
extern "C" int mahip_bgzf_range_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, int rank, int world, void *out, size_t out_cap, mahip_bgzf_range_t *range, mahip_bgzf_info_t *info)
{
	return bgzf_range_run(c, -1, comp, ncomp, rank, world, out, out_cap, range, info);
}
extern "C" int mahip_bgzf_last(mahip_ctx_t *c, mahip_bgzf_info_t *out) { *out = c->bgzf_last; return 0; }
extern "C" void mahip_bgzf_note(mahip_ctx_t *c, const mahip_bgzf_info_t *in) { c->bgzf_last = *in; }
extern "C" const char *mahip_bgzf_reason_name(int reason)
{
	static const char *const nm[] = {"ok", "not a BGZF file", "a member without a BC subfield", "a member runs past the end of the file", "trailing bytes behind the last member", "a header flag that is not handled",
	                                 "a member of more than 65536 bytes", "block type 3", "stored block: LEN does not match NLEN", "invalid code lengths", "invalid symbol", "a distance reaches in front of the member",
	                                 "more output than ISIZE", "the deflate bytes end early", "less output than ISIZE", "CRC mismatch", "not enough device memory", "not a regular file", "MA_BGZF_HOST is set", "no text"};
	return reason >= 0 && reason < (int)(sizeof(nm) / sizeof(nm[0])) ? nm[reason] : "?";
}

// ================================================================================================ plain gzip input, inflated on the device
// A member is ONE deflate stream (concatenated members: one stream each, found by k_gz_member_scan / k_gz_heads): what BGZF's headers give away -- where a block starts, how many bytes a piece inflates to, what the 32 KiB in front of a
// piece held -- is found here.  include/mahip.h has the scheme; gzip_core.h the per-lane header test and the wave's decode loop in its two forms.
#include "gzip_core.h"
#include <algorithm>
#include <vector>

#define GZ_CNT_WAVES 4u    // k_gz_sync_count: chunks per workgroup (tables only: 4 x 5.6 KiB of LDS)
#define GZ_DEC_WAVES 2u    // k_gz_decode: items per workgroup (2 x sizeof(GzLds) = 137 KiB of the CU's 160 KiB)
#define GZ_TILE 4096u      // k_gz_resolve: text bytes per workgroup
#define GZ_CRC_PIECE 65536u
#define GZ_CHUNK_MAX ((size_t)16 << 20) // (GZ_SPAN_MAX + 2) chunks + GZ_BLOCK_MAX stay below 2^32 / 8: a wave's local BIT positions fit 32 bits with room
struct gz_chain_t { uint64_t sync_bit, end_bit, out_off, out_len, base; }; // one item of the chain; bits of the payload; base: where its member's text starts
struct gz_piece_t { uint64_t text_off, behind; uint32_t size, member; }; // k_gz_crc: a piece of ONE member's text; the bytes of that member's text behind the piece

// the input a wave whose chunk starts at byte0 of the payload may read
__device__ __forceinline__ uint32_t gz_in_len(uint64_t payload_len, uint64_t byte0, uint64_t C)
{
	const uint64_t rest = payload_len - byte0, cap = (uint64_t)(GZ_SPAN_MAX + 2) * C + GZ_BLOCK_MAX;
	return (uint32_t)(rest < cap ? rest : cap);
}
__device__ __forceinline__ void gz_state(InfState &s, const uint8_t *in, uint32_t in_len, unsigned lane)
{
	s.in = in; s.out = nullptr; s.in_len = in_len; s.isize = 0; s.ip = s.lp = s.op = s.fp = 0; s.bitbuf = 0; s.bitcnt = 0; s.err = INF_OK; s.fixed = 0; s.lane = lane;
	s.nblk[0] = s.nblk[1] = s.nblk[2] = 0;
}
__device__ __forceinline__ uint32_t gz_reason(uint32_t st) { return st == GZ_NO_SYNC ? (uint32_t)MAHIP_GZIP_NO_SYNC : (uint32_t)MAHIP_GZIP_BAD_BTYPE + st - 1; }

// The count pass of one wave whose coordinates are chunk k's.  known >= 0: the item starts at that local bit (chunk 0's bit 0; the first bit behind a member's
// header) and is not confirmed.  SEARCH and known < 0: the wave tries the chunk's own bits, 64 consecutive ones a round (one a lane: gz_holds), and
// confirms the survivors in ascending order by decoding the block (gz_item); the first confirmed one is the chunk's start.  Either way the decode goes on from
// there, counting, to the item's end.  Returns the item's row (sync_bit -1: no start found).  TERMINATION: the search visits each of the chunk's <= 8 C bits
// once, each candidate's trial and the item's decode consume input that is bounded by gz_in_len.  BOUNDS: the payload is read below byte0 + in_len <=
// payload_len only; nothing is written.
template <bool SEARCH> __device__ __forceinline__ mahip_gzip_item_t gz_count(const uint8_t *__restrict__ payload, uint64_t payload_len, uint64_t C, uint64_t k, int64_t known, InfTabs &tab,
                                                                             GzCand *cand, unsigned lane)
{
	const uint64_t byte0 = k * C, CB = C * 8;
	InfState s;
	gz_state(s, payload + byte0, gz_in_len(payload_len, byte0, C), lane);
	GzOut o;
	o.op = o.fp = o.lim = o.before = 0; o.out = nullptr;
	uint64_t start = 0, end = 0;
	uint32_t st = GZ_UNCONFIRMED, fin = 0, nblk[3] = {0, 0, 0};
	if (!SEARCH || known >= 0) { start = (uint64_t)known; st = gz_item<false>(s, tab, nullptr, o, start, CB, 0, false, &end, &fin, nblk); }
	else {
		const uint64_t own_bits = payload_len - byte0 < C ? (payload_len - byte0) * 8 : CB;
		for (uint64_t base = 0; base < own_bits && st == GZ_UNCONFIRMED; base += 64) {
			const uint64_t bit = base + lane;
			uint64_t m = wv_ballot(bit < own_bits && gz_holds(s.in, s.in_len, bit, cand->cnt[lane], cand->sym[lane]));
			while (m) {
				start = base + (uint64_t)(__ffsll((long long)m) - 1);
				m &= m - 1;
				o.op = 0;
				st = gz_item<false>(s, tab, nullptr, o, start, CB, 0, true, &end, &fin, nblk);
				if (st != GZ_UNCONFIRMED) break;
			}
		}
	}
	mahip_gzip_item_t r;
	if (st == GZ_UNCONFIRMED) { r.sync_bit = -1; r.end_bit = 0; r.out_len = 0; r.status = 0; r.flags = 0; }
	else { r.sync_bit = (int64_t)(byte0 * 8 + start); r.end_bit = byte0 * 8 + end; r.out_len = o.op; r.status = st ? gz_reason(st) : 0u; r.flags = fin ? MAHIP_GZIP_SAW_FINAL : 0u; }
	return r;
}

// One wave per chunk: chunk 0 starts at bit 0, every other chunk looks for its first block start (gz_count).  One row is written, rows[k], k < n_chunks.
__global__ __launch_bounds__(256) void k_gz_sync_count(const uint8_t *__restrict__ payload, uint64_t payload_len, uint64_t C, uint64_t n_chunks, mahip_gzip_item_t *__restrict__ rows)
{
	__shared__ InfTabs s_tab[GZ_CNT_WAVES];
	__shared__ GzCand s_cand[GZ_CNT_WAVES];
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t k = (uint64_t)blockIdx.x * GZ_CNT_WAVES + wave;
	if (k >= n_chunks) return; // the whole wave; nothing below waits for another wave
	const mahip_gzip_item_t r = gz_count<true>(payload, payload_len, C, k, k == 0 ? 0 : -1, s_tab[wave], &s_cand[wave], lane);
	if (lane == 0) rows[k] = r;
}

// Concatenated members (include/mahip.h).  Every byte position p in [from, nbytes - 4] whose four bytes read 1f 8b 08 FLG with FLG's bits 5..7 clear goes
// into list[] (in any order: the host sorts it); *count = how many there are, which may exceed cap -- nothing is written at or behind list[cap].  A lane takes
// the 4 positions of one aligned 32-bit word (it loads that word and the next), a wave 256 consecutive positions; a ballot says whether the wave has a hit at
// all (it hardly ever has), and then ONE atomic of lane 0 reserves the wave's cells.  TERMINATION: a counted grid-stride loop, the same trip count for every
// lane of a wave.  BOUNDS: comp is read below nbytes only (word loads where both words lie below it and comp is word-aligned, else bytewise).
__global__ __launch_bounds__(256) void k_gz_member_scan(const uint8_t *__restrict__ comp, uint64_t nbytes, uint64_t from, uint64_t cap, uint64_t *__restrict__ list,
                                                        unsigned long long *__restrict__ count)
{
	const unsigned lane = threadIdx.x & 63;
	const uint64_t n_words = (nbytes + 3) / 4, stride = (uint64_t)gridDim.x * 256;
	const bool aligned = ((uintptr_t)comp & 3u) == 0;
	const uint32_t *w32 = (const uint32_t*)comp;
	for (uint64_t base = ((uint64_t)blockIdx.x * 256 + threadIdx.x) - lane; base < n_words; base += stride) {
		const uint64_t i = base + lane, b = 4 * i;
		uint64_t v = 0;
		if (aligned && b + 8 <= nbytes) v = (uint64_t)w32[i] | (uint64_t)w32[i + 1] << 32;
		else for (uint32_t q = 0; q < 8; ++q) if (b + q < nbytes) v |= (uint64_t)comp[b + q] << (8 * q);
		uint32_t hm = 0;
		for (uint32_t q = 0; q < 4; ++q) {
			const uint64_t p = b + q;
			if (p >= from && p + 4 <= nbytes && ((uint32_t)(v >> (8 * q)) & 0xe0ffffffu) == 0x00088b1fu) hm |= 1u << q;
		}
		const uint64_t any = wv_ballot(hm != 0);
		if (any == 0) continue; // (the whole wave)
		const uint32_t mine = (uint32_t)__popc(hm);
		uint32_t before = 0, total = 0;
		for (uint64_t m = any; m; m &= m - 1) { // the lanes with a hit, ascending: a handful at the most
			const unsigned l = (unsigned)(__ffsll((long long)m) - 1);
			const uint32_t n = (uint32_t)__shfl((int)mine, (int)l, 64);
			if (l < lane) before += n;
			total += n;
		}
		unsigned long long at = 0;
		if (lane == 0) at = atomicAdd(count, (unsigned long long)total);
		const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)at, 0, 64), hi = (uint32_t)__shfl((int)(uint32_t)(at >> 32), 0, 64);
		uint64_t cell = ((uint64_t)hi << 32 | lo) + before;
		for (uint32_t q = 0; q < 4; ++q)
			if (hm >> q & 1u) { if (cell < cap) list[cell] = b + q; ++cell; }
	}
}

// One wave per candidate whose header parsed: the count pass from the first bit behind that header (head_bit[h], a bit of the payload), in the coordinates of
// the chunk that bit lies in -- what k_gz_sync_count does for chunk 0, with the same limits (GZ_SPAN_MAX, gz_in_len).  Nothing is confirmed: whether a member
// starts there the chain decides.  TERMINATION and BOUNDS: gz_count's; one row is written, rows[h], h < n_heads.
__global__ __launch_bounds__(256) void k_gz_heads(const uint8_t *__restrict__ payload, uint64_t payload_len, uint64_t C, const uint64_t *__restrict__ head_bit, uint64_t n_heads,
                                                  mahip_gzip_item_t *__restrict__ rows)
{
	__shared__ InfTabs s_tab[GZ_CNT_WAVES];
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t h = (uint64_t)blockIdx.x * GZ_CNT_WAVES + wave;
	if (h >= n_heads) return; // the whole wave
	const uint64_t bit = head_bit[h], k = bit / (C * 8);
	const mahip_gzip_item_t r = gz_count<false>(payload, payload_len, C, k, (int64_t)(bit - k * C * 8), s_tab[wave], nullptr, lane);
	if (lane == 0) rows[h] = r;
}

enum { GZ_RES_BAD = 0, GZ_RES_STORED, GZ_RES_FIXED, GZ_RES_DYNAMIC, GZ_RES_CAND, GZ_RES_WORDS = 8 }; // res[GZ_RES_BAD] = min over the items with a status of item << 8 | status; res[GZ_RES_CAND]: k_gz_member_scan's count

// One wave per chain item: the decode of the count pass again, now writing 16-bit symbols at sym[out_off ..] through the LDS ring of the last 32768 symbols.
// It stops where the count pass stopped (end_bit) after as many symbols (out_len): anything else is a status.  BOUNDS: sym is written at out_off + p, p <
// out_len, only (gz_codes / gz_stored check before they write, gz_flush writes what they produced).
__global__ __launch_bounds__(128) void k_gz_decode(const uint8_t *__restrict__ payload, uint64_t payload_len, uint64_t C, const gz_chain_t *__restrict__ chain, uint64_t n_items,
                                                   uint16_t *__restrict__ sym, unsigned long long *__restrict__ res)
{
	__shared__ GzLds s_lds[GZ_DEC_WAVES];
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t j = (uint64_t)blockIdx.x * GZ_DEC_WAVES + wave;
	if (j >= n_items) return;
	const gz_chain_t it = chain[j];
	const uint64_t CB = C * 8, k = it.sync_bit / CB, byte0 = k * C;
	InfState s;
	gz_state(s, payload + byte0, gz_in_len(payload_len, byte0, C), lane);
	GzOut o;
	o.op = o.fp = 0; o.lim = it.out_len; o.before = it.out_off - it.base; o.out = sym + it.out_off; // (before: the text of the item's OWN member in front of it)
	uint64_t end = 0;
	uint32_t fin = 0, nblk[3] = {0, 0, 0};
	uint32_t st = gz_item<true>(s, s_lds[wave], s_lds[wave].ring, o, it.sync_bit - k * CB, CB, it.end_bit - k * CB, false, &end, &fin, nblk);
	if (!st && (o.op != it.out_len || end != it.end_bit - k * CB)) st = INF_OUT_SHORT;
	gz_flush(s, s_lds[wave].ring, o);
	if (lane == 0) {
		if (st) atomicMin(res + GZ_RES_BAD, (unsigned long long)(j << 8 | gz_reason(st)));
		if (nblk[0]) atomicAdd(res + GZ_RES_STORED, (unsigned long long)nblk[0]);
		if (nblk[1]) atomicAdd(res + GZ_RES_FIXED, (unsigned long long)nblk[1]);
		if (nblk[2]) atomicAdd(res + GZ_RES_DYNAMIC, (unsigned long long)nblk[2]);
	}
}

// One workgroup per MEMBER (item0[m] .. item0[m + 1] are its items), the only serial step, serial within a member only: the window of a member's first item
// is the window in front of its stream, all zero and never referenced (k_gz_decode refuses a reach in front of the member, it knows how much of the member's
// text lies in front of an item); W[j + 1] = the last 32768 cells of W[j] followed by item j's resolved symbols.  An item of fewer than 32768 bytes passes older
// cells on.  BOUNDS: W holds n_items windows and a workgroup writes those of its own member's items only; sym is read at out_off + [out_len - 32768, out_len)
// clipped to the item.
__global__ __launch_bounds__(256) void k_gz_windows(const gz_chain_t *__restrict__ chain, const uint64_t *__restrict__ item0, const uint16_t *__restrict__ sym, uint8_t *W)
{
	const uint64_t j0 = item0[blockIdx.x], j1 = item0[blockIdx.x + 1];
	if (j0 >= j1) return; // (the whole workgroup)
	for (uint32_t i = threadIdx.x; i < GZ_WIN; i += 256) W[j0 * GZ_WIN + i] = 0;
	__syncthreads();
	for (uint64_t j = j0; j + 1 < j1; ++j) {
		const uint64_t off = chain[j].out_off, n = chain[j].out_len;
		const uint8_t *w0 = W + j * GZ_WIN;
		uint8_t *w1 = W + (j + 1) * GZ_WIN;
		for (uint32_t i = threadIdx.x; i < GZ_WIN; i += 256) {
			uint8_t v;
			if (n + i >= GZ_WIN) { const uint16_t sy = sym[off + (n + i - GZ_WIN)]; v = sy < 256 ? (uint8_t)sy : w0[sy & (GZ_WIN - 1)]; }
			else v = w0[i + n];
			w1[i] = v;
		}
		__syncthreads(); // W[j + 1] is complete (and visible to this workgroup) before it is read
	}
}

// text[p] = the symbol at p, or the cell it names in its item's window.  A workgroup takes GZ_TILE consecutive bytes; the item of a byte is the LAST one whose
// out_off is not behind it (items without output share their successor's offset).
__global__ __launch_bounds__(256) void k_gz_resolve(const gz_chain_t *__restrict__ chain, uint64_t n_items, const uint16_t *__restrict__ sym, const uint8_t *__restrict__ W,
                                                    uint8_t *__restrict__ text, uint64_t total)
{
	const uint64_t t0 = (uint64_t)blockIdx.x * GZ_TILE;
	if (t0 >= total) return;
	uint64_t lo = 0, hi = n_items; // chain[lo].out_off <= t0 < chain[hi].out_off (chain[n_items].out_off = total)
	while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (chain[mid].out_off <= t0) lo = mid; else hi = mid; }
	uint64_t j = lo;
	for (uint32_t k = threadIdx.x; k < GZ_TILE; k += 256) {
		const uint64_t p = t0 + k;
		if (p >= total) break;
		while (j + 1 < n_items && chain[j + 1].out_off <= p) ++j;
		const uint16_t sy = sym[p];
		text[p] = sy < 256 ? (uint8_t)sy : W[j * GZ_WIN + (sy & (GZ_WIN - 1))];
	}
}

// one wave per piece of the table (at most GZ_CRC_PIECE bytes of ONE member's text), as k_bgzf_crc per member; pc[piece] = the piece's CRC moved in front of all
// the text of its member that lies behind it (x^(8 n) with a 64-bit n): the XOR of a member's pc[] is the CRC of its text
__global__ __launch_bounds__(256) void k_gz_crc(const uint8_t *__restrict__ text, const gz_piece_t *__restrict__ pieces, uint64_t n_pieces, uint32_t *__restrict__ pc)
{
	__shared__ uint32_t s_crc[256];
	{
		uint32_t v = threadIdx.x;
		for (int k = 0; k < 8; ++k) v = v & 1u ? (v >> 1) ^ INF_CRC_POLY : v >> 1;
		s_crc[threadIdx.x] = v;
	}
	__syncthreads();
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t m = (uint64_t)blockIdx.x * 4 + wave;
	if (m >= n_pieces) return;
	const gz_piece_t pp = pieces[m];
	const uint32_t size = pp.size;
	const uint8_t *t = text + pp.text_off;
	const uint32_t piece = (size + 63u) / 64u;
	const uint32_t b = lane * piece < size ? lane * piece : size, e = b + piece < size ? b + piece : size;
	uint32_t crc = 0xffffffffu;
	for (uint32_t p = b; p < e; ++p) crc = s_crc[(crc ^ t[p]) & 255u] ^ (crc >> 8);
	crc = ~crc;
	crc = inf_mulmod(crc, inf_xpow8(size - e));
	for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
	if (lane == 0) pc[m] = inf_mulmod(crc, inf_xpow8_64(pp.behind));
}

extern "C" int ma_gzip_head_at(int fd, const void *mem, uint64_t nbytes, uint64_t off, uint64_t *hdr_len);
extern "C" int ma_gzip_trailer_at(int fd, const void *mem, uint64_t nbytes, uint64_t off, uint32_t *crc, uint32_t *isize);
extern "C" size_t ma_gzip_chunk(void);
extern "C" size_t ma_gzip_cand_cap(void);

static void gzip_report(mahip_ctx *c, const mahip_gzip_info_t *info, const mahip_gzip_members_info_t *mi)
{
	c->gzip_last = *info;
	if (mi) c->gzip_mlast = *mi; else { memset(&c->gzip_mlast, 0, sizeof(c->gzip_mlast)); c->gzip_mlast.bad_member = -1; }
	if (ma_timing_level() < 1) return;
	fprintf(stderr, "[T::gzip] reader=%s reason=%d (%s) item=%lld chunks=%llu (%llu B each, %llu synced) items=%llu %.1f MB -> %.1f MB: upload %.3f sync+count %.3f decode %.3f windows %.3f resolve %.3f crc %.3f ms\n",
	        info->reader == MAHIP_BGZF_DEVICE ? "device" : "host", info->reason, mahip_gzip_reason_name(info->reason), (long long)info->first_bad_item, (unsigned long long)info->n_chunks,
	        (unsigned long long)info->chunk, (unsigned long long)info->n_synced, (unsigned long long)info->n_items, (double)info->comp_bytes / 1e6, (double)info->text_bytes / 1e6, info->laps_ms[0],
	        info->laps_ms[1], info->laps_ms[2], info->laps_ms[3], info->laps_ms[4], info->laps_ms[5]);
	if (mi) fprintf(stderr, "[T::gzip_members] members=%llu candidates=%llu heads=%llu member=%lld: scan %.3f heads %.3f ms\n", (unsigned long long)mi->n_members, (unsigned long long)mi->n_candidates,
	                (unsigned long long)mi->n_heads, (long long)mi->bad_member, mi->laps_ms[0], mi->laps_ms[1]);
}

struct gz_head_t { uint64_t pos, hdr_len; }; // a candidate whose header parsed: where it starts in the file
struct gz_src_t { int fd; const void *mem; uint64_t nbytes; };

// the rows -> the chain (host; a few thousand rows).  Follows end_bit from chunk 0; where a member's final block ends it looks for the next member among the
// candidates' head rows (include/mahip.h; none when the caller takes one member only).  Returns the reason, -1 on a read error; *bad = the chain item it is
// about, *bad_member the member.  chain has room for n_chunks + n_heads + 1 items, mrows for n_heads + 1 members.
static int gzip_chain(const gz_src_t &src, mahip_gzip_item_t *rows, uint64_t n_chunks, uint64_t CB, uint64_t hdr0, const gz_head_t *heads, mahip_gzip_item_t *head_rows, uint64_t n_heads,
                      gz_chain_t *chain, uint64_t *n_items, uint64_t *total, int64_t *bad, mahip_gzip_member_t *mrows, uint64_t *n_members, int64_t *bad_member)
{
	const uint64_t nbytes = src.nbytes;
	uint64_t cur = 0, n = 0, tot = 0, m = 0, base = 0;
	int reason = MAHIP_GZIP_OK;
	mahip_gzip_item_t *r = &rows[0];
	*bad = *bad_member = -1;
	memset(&mrows[0], 0, sizeof(mrows[0]));
	mrows[0].hdr_len = hdr0;
	for (;;) {
		if (n >= n_chunks + n_heads) { reason = MAHIP_GZIP_SYNC_MISMATCH; *bad = (int64_t)n; *bad_member = (int64_t)m; break; } // (cannot be: every row is visited once at the most)
		r->flags |= MAHIP_GZIP_ON_CHAIN;
		chain[n].sync_bit = (uint64_t)r->sync_bit; chain[n].end_bit = r->end_bit; chain[n].out_off = tot; chain[n].out_len = r->out_len; chain[n].base = base;
		++n; ++mrows[m].n_items;
		if (r->status) { reason = (int)r->status; *bad = (int64_t)n - 1; *bad_member = (int64_t)m; break; }
		tot += r->out_len;
		mrows[m].text_len = tot - base;
		if (r->flags & MAHIP_GZIP_SAW_FINAL) { // the member ends here: its trailer, and then the end of the file or the next member
			const uint64_t q = hdr0 + (r->end_bit + 7) / 8 + 8;
			uint64_t h = n_heads;
			if (q < nbytes) {
				uint64_t lo = 0, hi = n_heads;
				while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (heads[mid].pos < q) lo = mid + 1; else hi = mid; }
				if (lo < n_heads && heads[lo].pos == q) h = lo;
			}
			if (q != nbytes && h == n_heads) { reason = MAHIP_GZIP_MULTI_MEMBER; *bad = (int64_t)n - 1; *bad_member = (int64_t)m; break; }
			if (ma_gzip_trailer_at(src.fd, src.mem, nbytes, q - 8, &mrows[m].crc, &mrows[m].isize) != 0) return -1;
			if ((uint32_t)(tot - base) != mrows[m].isize) { reason = MAHIP_GZIP_ISIZE; *bad_member = (int64_t)m; break; }
			if (q == nbytes) break;
			++m; base = tot;
			memset(&mrows[m], 0, sizeof(mrows[m]));
			mrows[m].comp_off = q; mrows[m].hdr_len = heads[h].hdr_len; mrows[m].text_off = tot;
			r = &head_rows[h]; // (a head item may end in the chunk it starts in: a member may be far smaller than a chunk)
			cur = (uint64_t)r->sync_bit / CB;
			continue;
		}
		const uint64_t next = r->end_bit / CB;
		if (next <= cur || next >= n_chunks || rows[next].sync_bit != (int64_t)r->end_bit) { reason = MAHIP_GZIP_SYNC_MISMATCH; *bad = (int64_t)n; *bad_member = (int64_t)m; break; } // (the first two cannot be: an item that is not the last of its member ends at a block start in a later chunk)
		cur = next; r = &rows[next];
	}
	*n_items = n; *total = tot; *n_members = m + 1;
	return reason;
}

// as bgzf_run.  chunk 0: MA_GZIP_CHUNK or the default.  members: concatenated members are taken (include/mahip.h), else the first must be the only one.
static int gzip_run(mahip_ctx *c, int fd, const void *mem, size_t nbytes, int target, size_t chunk, void *out, size_t out_cap, mahip_gzip_info_t *info, bool members)
{
	HIPCHK(hipSetDevice(c->dev));
	memset(info, 0, sizeof(*info));
	info->reader = MAHIP_BGZF_HOST; info->first_bad_item = -1; info->comp_bytes = nbytes;
	if (chunk == 0) chunk = ma_gzip_chunk();
	if (chunk < 1024 || chunk > GZ_CHUNK_MAX || (chunk & (chunk - 1))) { mahip_set_error("mahip_gzip_load: chunk size %zu is not a power of two in 1024 .. %zu", chunk, GZ_CHUNK_MAX); return -1; }
	info->chunk = chunk;
	free(c->gzip_rows); c->gzip_rows = nullptr; c->gzip_n_rows = 0;
	free(c->gzip_members); c->gzip_members = nullptr; c->gzip_n_members = 0;
	mahip_gzip_members_info_t minfo;
	memset(&minfo, 0, sizeof(minfo));
	minfo.bad_member = -1; minfo.cand_cap = members ? ma_gzip_cand_cap() : 0;
	const mahip_gzip_members_info_t *mi = members ? &minfo : nullptr;
	const gz_src_t src = {fd, mem, nbytes};
	uint64_t hdr_len = 0;
	double t0 = bg_now(), t1;
	const int hr = ma_gzip_head_at(fd, mem, nbytes, 0, &hdr_len);
	if (hr < 0) { mahip_set_error("mahip_gzip_load: cannot read the compressed input"); return -1; }
	info->reason = hr;
	if (hr != MAHIP_GZIP_OK) { gzip_report(c, info, mi); return 0; }
	const uint64_t payload_len = nbytes - hdr_len - 8, n_chunks = payload_len ? (payload_len + chunk - 1) / chunk : 1, CB = (uint64_t)chunk * 8;
	info->n_chunks = n_chunks;
	DevBuf d_comp, d_rows, d_chain, d_sym, d_W, d_pc, d_res, d_own, d_cand, d_hbit, d_hrows, d_item0, d_pieces;
	void *d_text = nullptr;
	mahip_gzip_item_t *rows = (mahip_gzip_item_t*)malloc((size_t)n_chunks * sizeof(*rows));
	std::vector<gz_chain_t> chain;
	std::vector<uint64_t> cand, hbit, item0;
	std::vector<gz_head_t> heads;
	std::vector<mahip_gzip_item_t> head_rows;
	std::vector<mahip_gzip_member_t> mrows;
	std::vector<gz_piece_t> pieces;
	std::vector<uint32_t> h_pc;
	uint64_t n_items = 0, total = 0, n_pieces = 0, n_members = 0;
	int rc = 0;
	bool said = false; // the error message is set
	if (rows == nullptr) { mahip_set_error("mahip_gzip_load: out of host memory"); return -1; }
	if (dev_reserve(c, d_comp, nbytes + 64) != 0 || dev_reserve(c, d_rows, (size_t)n_chunks * sizeof(*rows)) != 0 || dev_reserve(c, d_res, GZ_RES_WORDS * 8) != 0 ||
	    (members && dev_reserve(c, d_cand, (size_t)minfo.cand_cap * 8) != 0)) info->reason = MAHIP_GZIP_NOMEM;
	do { // (one pass; `break` with rc = -1: a real error; with rc = 0: done, info->reason says how)
		if (info->reason != MAHIP_GZIP_OK) break;
		const uint8_t *payload = (const uint8_t*)d_comp.p + hdr_len;
		rc = -1;
		if ((fd >= 0 ? xfer_from_fd(c, d_comp.p, fd, nbytes) : xfer_copy(c, d_comp.p, (void*)mem, nbytes, 1)) != 0) break;
		if (hipMemsetAsync(d_res.p, 0, GZ_RES_WORDS * 8, c->st) != hipSuccess || hipMemsetAsync(d_res.p, 0xff, 8, c->st) != hipSuccess) break;
		if (hipStreamSynchronize(c->st) != hipSuccess) break;
		info->laps_ms[0] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		if (members) { // where may a further member start?  Candidates from the device, their headers read here
			unsigned long long n_cand = 0;
			{
				const uint64_t n_words = (nbytes + 3) / 4, want = (n_words + 255) / 256;
				ProfScope ps(c, "k_gz_member_scan", (double)nbytes);
				hipLaunchKernelGGL(k_gz_member_scan, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, c->st, (const uint8_t*)d_comp.p, (uint64_t)nbytes, hdr_len, (uint64_t)minfo.cand_cap,
				                   (uint64_t*)d_cand.p, P<unsigned long long>(d_res) + GZ_RES_CAND);
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipMemcpyAsync(&n_cand, P<unsigned long long>(d_res) + GZ_RES_CAND, 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
			minfo.n_candidates = n_cand;
			if (n_cand > minfo.cand_cap) { info->reason = MAHIP_GZIP_TOO_MANY_CANDIDATES; rc = 0; break; }
			cand.resize((size_t)n_cand);
			if (n_cand && (hipMemcpyAsync(cand.data(), d_cand.p, (size_t)n_cand * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)) break;
			std::sort(cand.begin(), cand.end());
			bool io = false;
			for (uint64_t p : cand) {
				uint64_t hl = 0;
				const int r = ma_gzip_head_at(fd, mem, nbytes, p, &hl);
				if (r < 0) { io = true; break; }
				if (r == MAHIP_GZIP_OK) { heads.push_back({p, hl}); hbit.push_back((p + hl - hdr_len) * 8); } // (p + hl + 8 <= nbytes: the bit lies in the payload, or is its end)
			}
			if (io) { mahip_set_error("mahip_gzip_load: cannot read the compressed input"); said = true; break; }
			minfo.n_heads = heads.size();
			minfo.laps_ms[0] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		}
		{
			ProfScope ps(c, "k_gz_sync_count", (double)payload_len);
			hipLaunchKernelGGL(k_gz_sync_count, dim3((unsigned)((n_chunks + GZ_CNT_WAVES - 1) / GZ_CNT_WAVES)), dim3(256), 0, c->st, payload, payload_len, (uint64_t)chunk, n_chunks, (mahip_gzip_item_t*)d_rows.p);
			if (hipGetLastError() != hipSuccess) break;
		}
		if (hipMemcpyAsync(rows, d_rows.p, (size_t)n_chunks * sizeof(*rows), hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
		for (uint64_t k = 0; k < n_chunks; ++k) info->n_synced += rows[k].sync_bit >= 0;
		if (!heads.empty()) { // the head items: one wave per candidate that may begin a member
			const uint64_t nh = heads.size();
			const double th = bg_now();
			head_rows.resize((size_t)nh);
			if (dev_reserve(c, d_hbit, (size_t)nh * 8) != 0 || dev_reserve(c, d_hrows, (size_t)nh * sizeof(mahip_gzip_item_t)) != 0) { info->reason = MAHIP_GZIP_NOMEM; rc = 0; break; }
			if (hipMemcpyAsync(d_hbit.p, hbit.data(), (size_t)nh * 8, hipMemcpyHostToDevice, c->st) != hipSuccess) break;
			{
				ProfScope ps(c, "k_gz_heads", (double)payload_len);
				hipLaunchKernelGGL(k_gz_heads, dim3((unsigned)((nh + GZ_CNT_WAVES - 1) / GZ_CNT_WAVES)), dim3(256), 0, c->st, payload, payload_len, (uint64_t)chunk, (const uint64_t*)d_hbit.p, nh, (mahip_gzip_item_t*)d_hrows.p);
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipMemcpyAsync(head_rows.data(), d_hrows.p, (size_t)nh * sizeof(mahip_gzip_item_t), hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
			minfo.laps_ms[1] = ((t1 = bg_now()) - th) * 1e3;
			t0 += t1 - th; // (the lap below is the chunks' pass and the chain, as ever)
		}
		chain.resize((size_t)(n_chunks + heads.size() + 1));
		mrows.resize(heads.size() + 1);
		{
			const int cr = gzip_chain(src, rows, n_chunks, CB, hdr_len, heads.data(), head_rows.data(), heads.size(), chain.data(), &n_items, &total, &info->first_bad_item, mrows.data(), &n_members, &minfo.bad_member);
			if (cr < 0) { mahip_set_error("mahip_gzip_load: cannot read the compressed input"); said = true; break; }
			info->reason = cr;
		}
		minfo.n_members = n_members;
		chain[n_items].sync_bit = chain[n_items].end_bit = 0; chain[n_items].out_off = total; chain[n_items].out_len = 0; chain[n_items].base = total;
		info->n_items = n_items; info->text_bytes = total;
		info->laps_ms[1] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		rc = 0;
		if (info->reason != MAHIP_GZIP_OK) break;
		// the text, the way the reader it is for reserves it (the PAF reader's cap, MA_PAF_MAX_BYTES, counts the inflated bytes)
		if (target == MAHIP_BGZF_PAF) { if (paf_text_reserve(c, (size_t)total, &d_text) != 0) { rc = -1; said = true; break; } }
		else if (target == MAHIP_BGZF_FASTX) {
			if (total == 0) { info->reason = MAHIP_GZIP_EMPTY; break; }
			if (fx_text_reserve(c, (size_t)total, &d_text) != 0) { info->reason = MAHIP_GZIP_NOMEM; break; }
		} else {
			if (out_cap < total) { mahip_set_error("mahip_gzip_inflate_mem: %llu bytes of text, room for %zu", (unsigned long long)total, out_cap); rc = -1; said = true; break; }
			if (dev_reserve(c, d_own, (size_t)total + 64) != 0) { info->reason = MAHIP_GZIP_NOMEM; break; }
			d_text = d_own.p;
		}
		// the members' first items, and the CRC's pieces: at most GZ_CRC_PIECE bytes, none across a member's end
		item0.resize((size_t)n_members + 1);
		item0[0] = 0;
		for (uint64_t m = 0; m < n_members; ++m) {
			item0[m + 1] = item0[m] + mrows[m].n_items;
			for (uint64_t o = 0; o < mrows[m].text_len; o += GZ_CRC_PIECE) {
				gz_piece_t pp;
				pp.size = mrows[m].text_len - o < GZ_CRC_PIECE ? (uint32_t)(mrows[m].text_len - o) : GZ_CRC_PIECE;
				pp.text_off = mrows[m].text_off + o; pp.behind = mrows[m].text_len - o - pp.size; pp.member = (uint32_t)m;
				pieces.push_back(pp);
			}
		}
		n_pieces = pieces.size();
		if (dev_reserve(c, d_chain, (size_t)(n_items + 1) * sizeof(gz_chain_t)) != 0 || dev_reserve(c, d_sym, 2 * (size_t)total + 64) != 0 || dev_reserve(c, d_W, (size_t)n_items * GZ_WIN) != 0 ||
		    dev_reserve(c, d_pc, (size_t)n_pieces * 4 + 64) != 0 || dev_reserve(c, d_item0, (size_t)(n_members + 1) * 8) != 0 || dev_reserve(c, d_pieces, (size_t)n_pieces * sizeof(gz_piece_t) + 64) != 0) {
			info->reason = MAHIP_GZIP_NOMEM; break;
		}
		h_pc.resize((size_t)n_pieces + 1);
		rc = -1;
		if (hipMemcpyAsync(d_chain.p, chain.data(), (size_t)(n_items + 1) * sizeof(gz_chain_t), hipMemcpyHostToDevice, c->st) != hipSuccess) break;
		if (hipMemcpyAsync(d_item0.p, item0.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, c->st) != hipSuccess) break;
		if (n_pieces && hipMemcpyAsync(d_pieces.p, pieces.data(), (size_t)n_pieces * sizeof(gz_piece_t), hipMemcpyHostToDevice, c->st) != hipSuccess) break;
		unsigned long long h_res[GZ_RES_WORDS];
		{
			ProfScope ps(c, "k_gz_decode", (double)payload_len + 2.0 * (double)total);
			hipLaunchKernelGGL(k_gz_decode, dim3((unsigned)((n_items + GZ_DEC_WAVES - 1) / GZ_DEC_WAVES)), dim3(128), 0, c->st, payload, payload_len, (uint64_t)chunk, (const gz_chain_t*)d_chain.p, n_items,
			                   (uint16_t*)d_sym.p, P<unsigned long long>(d_res));
			if (hipGetLastError() != hipSuccess) break;
		}
		if (hipMemcpyAsync(h_res, d_res.p, GZ_RES_WORDS * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
		info->laps_ms[2] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		info->n_stored = h_res[GZ_RES_STORED]; info->n_fixed = h_res[GZ_RES_FIXED]; info->n_dynamic = h_res[GZ_RES_DYNAMIC];
		if (h_res[GZ_RES_BAD] != ~0ull) {
			info->reason = (int)(h_res[GZ_RES_BAD] & 255u); info->first_bad_item = (int64_t)(h_res[GZ_RES_BAD] >> 8); rc = 0;
			for (uint64_t m = 0; m < n_members; ++m) if ((uint64_t)info->first_bad_item >= item0[m] && (uint64_t)info->first_bad_item < item0[m + 1]) minfo.bad_member = (int64_t)m;
			break;
		}
		{
			ProfScope ps(c, "k_gz_windows", 3.0 * (double)n_items * GZ_WIN);
			hipLaunchKernelGGL(k_gz_windows, dim3((unsigned)n_members), dim3(256), 0, c->st, (const gz_chain_t*)d_chain.p, (const uint64_t*)d_item0.p, (const uint16_t*)d_sym.p, (uint8_t*)d_W.p);
			if (hipGetLastError() != hipSuccess) break;
		}
		if (hipStreamSynchronize(c->st) != hipSuccess) break;
		info->laps_ms[3] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		if (total) {
			ProfScope ps(c, "k_gz_resolve", 3.0 * (double)total);
			hipLaunchKernelGGL(k_gz_resolve, dim3((unsigned)((total + GZ_TILE - 1) / GZ_TILE)), dim3(256), 0, c->st, (const gz_chain_t*)d_chain.p, n_items, (const uint16_t*)d_sym.p, (const uint8_t*)d_W.p,
			                   (uint8_t*)d_text, total);
			if (hipGetLastError() != hipSuccess) break;
		}
		if (hipStreamSynchronize(c->st) != hipSuccess) break;
		info->laps_ms[4] = ((t1 = bg_now()) - t0) * 1e3; t0 = t1;
		if (n_pieces) {
			{
				ProfScope ps(c, "k_gz_crc", (double)total);
				hipLaunchKernelGGL(k_gz_crc, dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, c->st, (const uint8_t*)d_text, (const gz_piece_t*)d_pieces.p, n_pieces, (uint32_t*)d_pc.p);
				if (hipGetLastError() != hipSuccess) break;
			}
			if (hipMemcpyAsync(h_pc.data(), d_pc.p, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) break;
		}
		info->laps_ms[5] = (bg_now() - t0) * 1e3;
		rc = 0;
		{ // every member's pieces against its own trailer (a member without text: no piece, CRC 0)
			std::vector<uint32_t> got((size_t)n_members, 0u);
			for (uint64_t k = 0; k < n_pieces; ++k) got[pieces[k].member] ^= h_pc[k];
			for (uint64_t m = 0; m < n_members && info->reason == MAHIP_GZIP_OK; ++m) if (got[m] != mrows[m].crc) { info->reason = MAHIP_GZIP_CRC; minfo.bad_member = (int64_t)m; }
		}
		if (info->reason != MAHIP_GZIP_OK) break;
		if (target == 0 && total) rc = xfer_copy(c, d_text, out, (size_t)total, 0);
	} while (0);
	if (rc != 0 && !said) mahip_set_error("mahip_gzip_load: upload, launch or copy failed (%s)", hipGetErrorString(hipGetLastError()));
	(void)hipStreamSynchronize(c->st);
	dev_free(c, d_comp); dev_free(c, d_rows); dev_free(c, d_chain); dev_free(c, d_sym); dev_free(c, d_W); dev_free(c, d_pc); dev_free(c, d_res); dev_free(c, d_own);
	dev_free(c, d_cand); dev_free(c, d_hbit); dev_free(c, d_hrows); dev_free(c, d_item0); dev_free(c, d_pieces);
	c->gzip_rows = rows; c->gzip_n_rows = info->laps_ms[1] > 0 ? n_chunks : 0; // (rows that were never downloaded are not rows)
	if (members && n_members) {
		c->gzip_members = (mahip_gzip_member_t*)malloc((size_t)n_members * sizeof(mahip_gzip_member_t));
		if (c->gzip_members) { memcpy(c->gzip_members, mrows.data(), (size_t)n_members * sizeof(mahip_gzip_member_t)); c->gzip_n_members = n_members; }
	}
	if (rc == 0 && info->reason == MAHIP_GZIP_OK) {
		info->reader = MAHIP_BGZF_DEVICE;
		if (target == MAHIP_BGZF_PAF) paf_text_loaded(c); else if (target == MAHIP_BGZF_FASTX) fx_text_loaded(c);
	} else { // nothing stays loaded: the caller inflates with zlib
		if (target == MAHIP_BGZF_PAF) (void)mahip_paf_release(c); else if (target == MAHIP_BGZF_FASTX) (void)mahip_fastx_release(c);
	}
	if (rc == 0) gzip_report(c, info, mi); else { c->gzip_last = *info; c->gzip_mlast = minfo; }
	return rc;
}

static int gzip_target_ok(int target, const char *who)
{
	if (target != MAHIP_BGZF_PAF && target != MAHIP_BGZF_FASTX) { mahip_set_error("%s: target %d", who, target); return -1; }
	return 0;
}
extern "C" int mahip_gzip_load_fd(mahip_ctx_t *c, int fd, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info)
{
	if (gzip_target_ok(target, "mahip_gzip_load_fd") != 0) return -1;
	return gzip_run(c, fd, nullptr, nbytes, target, chunk, nullptr, 0, info, false);
}
extern "C" int mahip_gzip_load_mem(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info)
{
	if (gzip_target_ok(target, "mahip_gzip_load_mem") != 0) return -1;
	return gzip_run(c, -1, comp, nbytes, target, chunk, nullptr, 0, info, false);
}
extern "C" int mahip_gzip_inflate_mem(mahip_ctx_t *c, const void *comp, size_t ncomp, size_t chunk, void *out, size_t out_cap, mahip_gzip_info_t *info) { return gzip_run(c, -1, comp, ncomp, 0, chunk, out, out_cap, info, false); }
extern "C" int mahip_gzip_load_fd_members(mahip_ctx_t *c, int fd, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info)
{
	if (gzip_target_ok(target, "mahip_gzip_load_fd_members") != 0) return -1;
	return gzip_run(c, fd, nullptr, nbytes, target, chunk, nullptr, 0, info, true);
}
extern "C" int mahip_gzip_load_mem_members(mahip_ctx_t *c, const void *comp, size_t nbytes, int target, size_t chunk, mahip_gzip_info_t *info)
{
	if (gzip_target_ok(target, "mahip_gzip_load_mem_members") != 0) return -1;
	return gzip_run(c, -1, comp, nbytes, target, chunk, nullptr, 0, info, true);
}
extern "C" int mahip_gzip_inflate_mem_members(mahip_ctx_t *c, const void *comp, size_t ncomp, size_t chunk, void *out, size_t out_cap, mahip_gzip_info_t *info) { return gzip_run(c, -1, comp, ncomp, 0, chunk, out, out_cap, info, true); }
extern "C" int mahip_gzip_last(mahip_ctx_t *c, mahip_gzip_info_t *out) { *out = c->gzip_last; return 0; }
extern "C" void mahip_gzip_note(mahip_ctx_t *c, const mahip_gzip_info_t *in) { c->gzip_last = *in; memset(&c->gzip_mlast, 0, sizeof(c->gzip_mlast)); c->gzip_mlast.bad_member = -1; }
extern "C" int mahip_gzip_members_last(mahip_ctx_t *c, mahip_gzip_members_info_t *out) { *out = c->gzip_mlast; return 0; }
extern "C" uint64_t mahip_gzip_items_download(mahip_ctx_t *c, mahip_gzip_item_t *out, uint64_t cap)
{
	const uint64_t n = c->gzip_n_rows < cap ? c->gzip_n_rows : cap;
	if (n) memcpy(out, c->gzip_rows, (size_t)n * sizeof(*out));
	return n;
}
extern "C" uint64_t mahip_gzip_members_download(mahip_ctx_t *c, mahip_gzip_member_t *out, uint64_t cap)
{
	const uint64_t n = c->gzip_n_members < cap ? c->gzip_n_members : cap;
	if (n) memcpy(out, c->gzip_members, (size_t)n * sizeof(*out));
	return n;
}
extern "C" const char *mahip_gzip_reason_name(int reason)
{
	static const char *const nm[] = {"ok", "not a gzip header this reader takes", "more than one member, or trailing bytes", "no block start within the span", "an item ends where the next does not start",
	                                 "the items' total is not ISIZE", "block type 3", "stored block: LEN does not match NLEN", "invalid code lengths", "invalid symbol", "a distance reaches in front of the stream",
	                                 "more output than counted", "the deflate bytes end early", "less output than counted", "CRC mismatch", "not enough device memory", "not a regular file", "MA_GZIP_DEVICE is off", "no text",
	                                 "more member candidates than the list holds"};
	return reason >= 0 && reason < (int)(sizeof(nm) / sizeof(nm[0])) ? nm[reason] : "?";
}
