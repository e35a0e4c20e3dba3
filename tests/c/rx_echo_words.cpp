// rx_echo_words.cpp -- the RX echo's shared statement (warpcore_amd/csrc/
// wc_rx_echo.h: run lengths, the scan, entry -> (socket, list position), the
// grid size, the payload copy) compiled for the host alone, so the lines the
// gfx950 kernel compiles are held against tests/rx_echo_model.py without a GPU
// (tests/test_rx_echo_words.py).
//
//   rx_echo_words map <in> <out>
// Input, per case (little-endian): uint64 n, uint32 ns, uint32 m, 256 uint64
// start entries, 256 uint16 map entries (ns count).  Output, per case: uint64
// E, uint32 grid, uint32 0, then for every j < E: uint32 s, uint32 0, uint64
// list position.  The scan runs as the kernel runs it: eight steps over two
// buffers, every element of a step from the buffer the step before wrote.
//
//   rx_echo_words copy
// Every source phase x every destination phase x the lengths 0 .. 49 and 1472
// through re::copy_lane, the sixteen lanes of a group one after another, on a
// checked memory (checked_mem.h): loads aligned and overlapping the source
// range, stores naturally aligned and inside the destination range; then the
// bytes are compared and the bytes around the destination must be untouched.
// Prints the number of cases.
#include "checked_mem.h"
#include "wc_rx_echo.h"

#include <vector>

namespace re = wc::re;
namespace rr = wc::rr;

static int run_map(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out)
        return 2;
    for (;;) {
        uint64_t n;
        uint32_t arg[2];
        static uint64_t start[256];
        static uint16_t map[256];
        if (fread(&n, 8, 1, in) != 1)
            break;
        if (fread(arg, 4, 2, in) != 2 || fread(start, 8, 256, in) != 256 ||
            fread(map, 2, 256, in) != 256)
            return 2;
        const uint32_t ns = arg[0], m = arg[1];
        if (ns > re::kMaxSocks)
            return 2;
        uint64_t S[2][re::kRuns];
        for (uint32_t t = 0; t < re::kRuns; ++t)
            S[0][t] = n != 0 && t < ns ? re::run_len(start[t], start[t + 1], n, map[t]) : 0ull;
        for (uint32_t s = 0; s < re::kScanSteps; ++s)
            for (uint32_t t = 0; t < re::kRuns; ++t)
                re::scan_step(S[s & 1u], S[(s + 1u) & 1u], t, 1u << s);
        const uint64_t *inc = S[re::kScanSteps & 1u];
        const uint64_t E = inc[re::kRuns - 1u];
        const uint32_t head[2] = {re::grid_of(m), 0u};
        fwrite(&E, 8, 1, out);
        fwrite(head, 4, 2, out);
        for (uint64_t j = 0; j < E; ++j) {
            const re::Where w = re::where_of(inc, ns, j);
            if (w.s >= ns) {
                fprintf(stderr, "entry %llu: socket %u of %u\n", (unsigned long long)j, w.s, ns);
                return 3;
            }
            const uint32_t sw[2] = {w.s, 0u};
            const uint64_t at = start[w.s] + w.pos;
            fwrite(sw, 4, 2, out);
            fwrite(&at, 8, 1, out);
        }
    }
    fclose(out);
    return 0;
}

static int run_copy()
{
    alignas(16) static uint8_t src[2048], dst[2048];
    std::vector<uint32_t> lens;
    for (uint32_t l = 0; l < 50; ++l)
        lens.push_back(l);
    lens.push_back(1472);
    uint32_t x = 12345u, cases = 0;
    for (uint32_t sp = 0; sp < 16; ++sp)
        for (uint32_t dp = 0; dp < 16; ++dp)
            for (uint32_t len : lens) {
                for (uint8_t &b : src)
                    b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
                memset(dst, 0xA5, sizeof dst);
                const uint64_t sa = (uint64_t)(uintptr_t)src + 32u + sp;
                const uint64_t dd = (uint64_t)(uintptr_t)dst + 32u + dp;
                CheckedMem128<rr::Quad> mem{{sa, sa + len, dd, dd + len, "payload", "the payload"}};
                for (uint32_t g = 0; g < re::kGroup; ++g)
                    re::copy_lane(mem, sa, dd, len, g);
                for (uint32_t k = 0; k < sizeof dst; ++k) {
                    const bool in = k >= 32u + dp && k < 32u + dp + len;
                    const uint8_t want = in ? src[32u + sp + (k - 32u - dp)] : 0xA5;
                    if (dst[k] != want) {
                        fprintf(stderr, "phases %u/%u, %u bytes: byte %d of the payload is wrong\n",
                                sp, dp, len, (int)k - (int)(32u + dp));
                        return 3;
                    }
                }
                ++cases;
            }
    printf("%u\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "copy"))
        return run_copy();
    if (argc == 4 && !strcmp(argv[1], "map"))
        return run_map(argv[2], argv[3]);
    return 2;
}
