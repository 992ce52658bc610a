// xfer_drive.cpp -- TEST INFRASTRUCTURE: the staged copy's worker threads (miniasm_amd/csrc/xfer.hip) driven by a stand-alone program, so that the CPU
// build can be run under the thread sanitizer (`make tsan`).  No kernel is launched: the stand-in runtime's fibers never run.  Its copies are memmoves done by the
// calling thread, so two workers whose slices overlap by one byte write the same destination byte from two threads: a reported race, even where the bytes agree.
//   upload, download and the file road at 2 W + 1 slices + 1 byte (worker 0 takes a slot a second time, the last slice is one byte) for W = 1, 3, 16
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "mahip.h"

static const size_t SLICE = (size_t)4 << 20;

static uint64_t mix(uint64_t z)
{
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

static void fill(uint8_t *p, size_t n, uint64_t seed)
{
	size_t i = 0;
	for (; i + 8 <= n; i += 8) { const uint64_t v = mix(seed + i / 8); memcpy(p + i, &v, 8); }
	for (; i < n; ++i) p[i] = (uint8_t)(mix(seed + i / 8) >> (8 * (i % 8)));
}

static int same(const uint8_t *got, const uint8_t *want, size_t n, int W, const char *what)
{
	if (memcmp(got, want, n) == 0) return 1;
	for (size_t i = 0; i < n; ++i)
		if (got[i] != want[i]) {
			fprintf(stderr, "%s, %d workers: byte %zu differs (slice %zu, slice %% workers = %zu)\n", what, W, i, i / SLICE, i / SLICE % (size_t)W);
			break;
		}
	return 0;
}

#define MUST(call) do { if ((call) != 0) { fprintf(stderr, "%s failed: %s\n", #call, mahip_strerror()); return 1; } } while (0)

int main(void)
{
	mahip_ctx_t *c = mahip_create(0, nullptr);
	if (!c) { fprintf(stderr, "mahip_create: %s\n", mahip_strerror()); return 1; }
	const int Ws[3] = {1, 3, 16};
	const size_t n_max = (2 * 16 + 1) * SLICE + 1, file_off = SLICE + 1;
	uint8_t *src = (uint8_t*)malloc(n_max), *dst = (uint8_t*)malloc(n_max);
	if (!src || !dst) return 1;
	char path[] = "/tmp/xfer_drive_XXXXXX";
	const int fd = mkstemp(path);
	if (fd < 0) { perror("mkstemp"); return 1; }
	unlink(path);
	for (int k = 0; k < 3; ++k) {
		const int W = Ws[k];
		const size_t n = (size_t)(2 * W + 1) * SLICE + 1;
		char num[16];
		snprintf(num, sizeof(num), "%d", W);
		setenv("MA_XFER_THREADS", num, 1);
		void *d = nullptr;
		mahip_xfer_info_t x;
		MUST(mahip_xbuf(c, 0, n, &d));
		fill(src, n, 1000 + (uint64_t)W);
		MUST(mahip_memcpy_h2d(c, d, src, n));
		MUST(mahip_xfer_last(c, &x));
		if (x.road != MAHIP_XFER_STAGED_MEM || x.workers != W || x.slices != (uint64_t)(2 * W + 2)) { fprintf(stderr, "upload: road %d, %d workers, %llu slices\n", x.road, x.workers, (unsigned long long)x.slices); return 1; }
		memset(dst, 0, n);
		MUST(mahip_memcpy_d2h(c, dst, d, n));
		if (!same(dst, src, n, W, "memory road")) return 1;
		fill(src, n, 2000 + (uint64_t)W); // the file road: other bytes, at an offset that is a multiple of nothing
		if (pwrite(fd, src, n, (off_t)file_off) != (ssize_t)n) { perror("pwrite"); return 1; }
		MUST(mahip_memcpy_fd2d(c, d, fd, file_off, n));
		MUST(mahip_xfer_last(c, &x));
		if (x.road != MAHIP_XFER_STAGED_FILE || x.workers != W) { fprintf(stderr, "file: road %d, %d workers\n", x.road, x.workers); return 1; }
		memset(dst, 0, n);
		MUST(mahip_memcpy_d2h(c, dst, d, n));
		if (!same(dst, src, n, W, "file road")) return 1;
	}
	close(fd);
	free(src); free(dst);
	mahip_destroy(c);
	printf("OK\n");
	return 0;
}
