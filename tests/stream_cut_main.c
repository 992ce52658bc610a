/* stream_cut_main.c -- the cut-and-carry reader of the streamed ingest (host/ingest_gpu.c: ma_cut_next) on its own, for a sanitizer build: a stand-alone
 * program that reads stdin (a pipe, in reads of at most `chunk` bytes) and cuts it into pieces of whole lines with a piece size of `piece` bytes.  It checks
 * what the parse relies on -- every piece but the last ends with a newline, only the last piece is flagged last, the pieces concatenated are the input (byte
 * count and FNV-1a hash, computed on the way in and on the way out) -- and prints "OK <pieces> <bytes> <longest piece>".
 *   gcc -g -fsanitize=address,undefined -static-libasan -Iinclude -Iminiasm_amd/host -Iminiasm_amd/csrc tests/stream_cut_main.c miniasm_amd/host/ingest_gpu.c \
 *       -Ltests/emu/_build -lminiasm_amd_emu -Wl,-rpath,$PWD/tests/emu/_build -lz -lpthread -o /tmp/stream_cut && head -c 300000 x.paf | /tmp/stream_cut 256 7
 * (the library only supplies what the rest of ingest_gpu.c refers to; nothing of it runs).  Never loaded into Python, never run on a GPU.
 * tests/test_stream_cut_cpu.py builds it so and drives it from a pipe, over piece and read sizes, against a model of the rule. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "ma_host.h"

typedef struct { size_t chunk; uint64_t n, h; } src_t;
static uint64_t fnv(uint64_t h, const char *p, size_t n) { size_t i; for (i = 0; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 0x100000001b3ull; return h; }
static long read_cb(void *v, char *dst, size_t want)
{
	src_t *s = (src_t*)v;
	ssize_t r = read(0, dst, want < s->chunk ? want : s->chunk); /* short reads on purpose: the reader must ask again */
	if (r > 0) { s->h = fnv(s->h, dst, (size_t)r); s->n += (uint64_t)r; }
	return (long)r;
}

int main(int argc, char **argv)
{
	src_t s = { argc > 2 ? (size_t)atol(argv[2]) : 4096, 0, 0xcbf29ce484222325ull };
	ma_cut_t k;
	char *buf = 0;
	size_t cap = 0, len = 0, longest = 0;
	uint64_t n = 0, h = 0xcbf29ce484222325ull, pieces = 0;
	int last = 0;
	memset(&k, 0, sizeof(k));
	k.piece = argc > 1 ? (size_t)atol(argv[1]) : 1024;
	k.read = read_cb; k.src = &s;
	while (!last) {
		if (ma_cut_next(&k, &buf, &cap, &len, &last) != 0) { fprintf(stderr, "out of memory\n"); return 2; }
		if (!last && (len == 0 || buf[len - 1] != '\n')) { fprintf(stderr, "piece %lu: %lu bytes, not whole lines\n", (unsigned long)pieces, (unsigned long)len); return 1; }
		h = fnv(h, buf, len); n += len; ++pieces;
		if (len > longest) longest = len;
	}
	free(buf); free(k.carry);
	if (n != s.n || h != s.h) { fprintf(stderr, "the pieces are not the input: %lu of %lu bytes\n", (unsigned long)n, (unsigned long)s.n); return 1; }
	printf("OK %lu %lu %lu\n", (unsigned long)pieces, (unsigned long)n, (unsigned long)longest);
	return 0;
}
