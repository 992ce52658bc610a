// tests/emu/lookback_selftest.cpp -- TEST INFRASTRUCTURE: sc_look_back (miniasm_amd/csrc/mahip_internal.hpp; the chained scan and graph.hip's one-pass arc
// compaction chain their tiles through it) on published words written BY HAND.  A look-back that needs a second step of 64 predecessors -- 64 published
// aggregates in a row, none of them an inclusive prefix yet -- is a matter of timing on the device and cannot happen in the CPU build's launches at all (at most
// 8 blocks are in flight there), so the scan tests never reach `look -= 64` on purpose.  Here one wave looks back over a state array that stands still.
#include "mahip_internal.hpp"

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

__global__ void k_look(const unsigned long long *state, uint32_t tile, uint32_t epoch, uint32_t *out)
{
	const uint32_t p = sc_look_back(state, tile, epoch, threadIdx.x);
	out[threadIdx.x] = p;
}

static uint32_t agg(uint32_t i) { return i * 0x9E3779B1u + 12345u; } // sums wrap 2^32

// tiles [0, tile): the ones in `incl` (ascending) know their inclusive prefix, the others their own sum only; -> what tile `tile` must find
static uint32_t run(unsigned long long *state, uint32_t *out, uint32_t tile, uint32_t epoch, const std::vector<uint32_t> &incl)
{
	uint32_t want = 0, last = 0;
	bool have = false;
	for (uint32_t i = 0; i < tile + 64; ++i) state[i] = sc_pack(epoch - 1, SC_INCL, 0xBAD00000u + i); // an older launch's words everywhere, behind the tile too
	for (uint32_t i = 0; i < tile; ++i) state[i] = sc_pack(epoch, SC_AGG, agg(i));
	for (uint32_t i : incl) { state[i] = sc_pack(epoch, SC_INCL, 0x51000000u + 977u * i); last = i; have = true; }
	if (have) { want = 0x51000000u + 977u * last; for (uint32_t i = last + 1; i < tile; ++i) want += agg(i); }
	hipLaunchKernelGGL(k_look, dim3(1), dim3(64), 0, nullptr, (const unsigned long long*)state, tile, epoch, out);
	for (unsigned l = 0; l < 64; ++l) EXPECT(out[l] == out[0]); // wv_sum_u32 leaves the sum in every lane
	const uint32_t got = out[0];
	if (got != want) printf("tile %u, nearest inclusive prefix at %u: got %#x, want %#x\n", tile, last, got, want);
	return got == want;
}

int main()
{
	unsigned long long *state;
	uint32_t *out;
	hipMalloc(&state, (4096 + 64) * 8);
	hipMalloc(&out, 64 * 4);
	const uint32_t epoch = 77;
	EXPECT(run(state, out, 1, epoch, {0}));              // tile 0 alone, lane 0
	EXPECT(run(state, out, 10, epoch, {3, 7}));          // the NEAREST inclusive prefix counts, older ones behind it do not
	EXPECT(run(state, out, 64, epoch, {0}));             // one step that ends at its last lane
	EXPECT(run(state, out, 65, epoch, {0}));             // 64 aggregates, then a second step of one word
	EXPECT(run(state, out, 65, epoch, {1}));             // ... or the first step's last lane after all
	EXPECT(run(state, out, 66, epoch, {0, 1}));          // second step: lane 0 ends it, tile 0 is not added
	EXPECT(run(state, out, 128, epoch, {0}));            // two full steps
	EXPECT(run(state, out, 129, epoch, {0}));            // three
	EXPECT(run(state, out, 130, epoch, {0, 2}));
	EXPECT(run(state, out, 4096, epoch, {5}));           // 64 steps (graph.hip chains more tiles than the scan does)
	EXPECT(run(state, out, 300, epoch, {100, 236, 237})); // the first step's lane 62
	hipFree(state);
	hipFree(out);
	printf("%s: %d failures\n", g_fail ? "FAILED" : "OK", g_fail);
	return g_fail != 0;
}
