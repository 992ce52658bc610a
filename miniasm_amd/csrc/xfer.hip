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
		HIPCHK(hipMemcpyAsync(to_device ? dev_ptr : host_ptr, to_device ? host_ptr : dev_ptr, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->st));
		HIPCHK(hipStreamSynchronize(c->st));
		return 0;
	}
	int W = xfer_workers(to_device);
	const size_t n_slices = (bytes + XF_SLOT - 1) / XF_SLOT;
	if ((size_t)W > n_slices) W = (int)n_slices;
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
	if (rc) { mahip_set_error("xfer_copy: staged copy failed (%s)", hipGetErrorString(hipGetLastError())); return -1; }
	return 0;
}

int xfer_copy(mahip_ctx *c, void *dev_ptr, void *host_ptr, size_t bytes, int to_device) { return xfer_run(c, dev_ptr, host_ptr, -1, bytes, to_device); }
// bytes [0, bytes) of an open file -> device memory
int xfer_from_fd(mahip_ctx *c, void *dev_ptr, int fd, size_t bytes) { return xfer_run(c, dev_ptr, nullptr, fd, bytes, 1); }
// bytes [off, off + bytes) of an open file -> device memory (a rank's own range of the text: host/ingest_sharded.c)
int xfer_from_fd_at(mahip_ctx *c, void *dev_ptr, int fd, size_t off, size_t bytes) { return xfer_run(c, dev_ptr, nullptr, fd, bytes, 1, off); }

extern "C" int mahip_memcpy_h2d(mahip_ctx_t *c, void *d_dst, const void *h_src, size_t bytes) { return xfer_copy(c, d_dst, (void*)h_src, bytes, 1); }
extern "C" int mahip_memcpy_d2h(mahip_ctx_t *c, void *h_dst, const void *d_src, size_t bytes) { return xfer_copy(c, (void*)d_src, h_dst, bytes, 0); }

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
extern "C" int mahip_bgzf_last(mahip_ctx_t *c, mahip_bgzf_info_t *out) { *out = c->bgzf_last; return 0; }
extern "C" void mahip_bgzf_note(mahip_ctx_t *c, const mahip_bgzf_info_t *in) { c->bgzf_last = *in; }
extern "C" const char *mahip_bgzf_reason_name(int reason)
{
	static const char *const nm[] = {"ok", "not a BGZF file", "a member without a BC subfield", "a member runs past the end of the file", "trailing bytes behind the last member", "a header flag that is not handled",
	                                 "a member of more than 65536 bytes", "block type 3", "stored block: LEN does not match NLEN", "invalid code lengths", "invalid symbol", "a distance reaches in front of the member",
	                                 "more output than ISIZE", "the deflate bytes end early", "less output than ISIZE", "CRC mismatch", "not enough device memory", "not a regular file", "MA_BGZF_HOST is set", "no text"};
	return reason >= 0 && reason < (int)(sizeof(nm) / sizeof(nm[0])) ? nm[reason] : "?";
}
