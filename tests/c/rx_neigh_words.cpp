// rx_neigh_words.cpp -- the RX neighbours' shared statement (warpcore_amd/csrc/
// wc_rx_neigh.h: decision chain, update record, reply dwords, the stores at
// any phase) compiled for the host alone and driven from a case file, so the
// lines the gfx950 kernels compile are held against tests/rx_neigh_model.py
// without a GPU (tests/test_rx_neigh_words.py).
//
// Input, per case (little-endian): the 844 table bytes, then uint32 action (the
// reply plan's byte), code (0xFFFFFFFF: the plan's own), slot_bytes, source
// phase, destination phase, flen, then flen frame bytes.
// Output, per case: uint32 code, out_len, the 24 record bytes, then a 256-byte
// region pre-filled with 0xA5 in which the reply starts at byte 16 +
// destination phase.  Every access is checked (checked_mem.h): loads aligned and
// overlapping the frame, stores naturally aligned and inside the reply.
#include "checked_mem.h"
#include "wc_rx_neigh.h"

namespace rn = wc::rn;
namespace rr = wc::rr;

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out)
        return 2;
    alignas(16) static uint8_t src[4096], region[256];
    for (;;) {
        uint32_t e[rr::kEngineWords], arg[6];
        if (fread(e, 4, rr::kEngineWords, in) != rr::kEngineWords)
            break;
        if (fread(arg, 4, 6, in) != 6)
            return 2;
        const uint32_t action = arg[0], force = arg[1], slot = arg[2], sp = arg[3], dp = arg[4],
                       flen = arg[5];
        if (flen > 2048 || sp > 15 || dp > 15)
            return 2;
        memset(src, 0x5A, sizeof src);
        uint8_t *fr = src + 16 + sp;
        if (fread(fr, 1, flen, in) != flen)
            return 2;
        uint8_t z[2048 + 96] = {}; // the frame alone, zeros behind it: what the chain may look at
        memcpy(z, fr, flen);

        // the plan, as k_rx_neigh_plan feeds the chain
        rn::Look f;
        f.action = action, f.flen = flen;
        f.f3 = le32(z + 12), f.f4 = le32(z + 16), f.f5 = le32(z + 20);
        f.tpa = le32(z + 38), f.b54 = z[54];
        uint32_t code = rn::chain_head(e, f);
        if (code == rn::kTarget) {
            if (flen < 78) {
                fprintf(stderr, "a target outside the frame\n");
                exit(3);
            }
            const uint32_t t[4] = {le32(z + 62), le32(z + 66), le32(z + 70), le32(z + 74)};
            code = rn::chain_tail(e, t);
        }

        // the record and the build, as the list kernels run them on the code byte they are handed
        const uint32_t use = force != 0xFFFFFFFFu ? force : code;
        const uint64_t fa = (uint64_t)(uintptr_t)fr, fend = fa + flen;
        const uint64_t da = (uint64_t)(uintptr_t)region + 16u + dp;
        memset(region, 0xA5, sizeof region);
        uint32_t u[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (rn::is_update(use))
            rn::record_of(CheckedMem{fa, fend, 0, 0}, fa, flen, use, u);
        uint32_t out_len = 0;
        if (rn::is_reply(use)) {
            // the bounds again, on their own: the stores may touch this much and no more
            const uint32_t len = use == rn::kArpIsAt ? 42u : 86u;
            const bool ok = flen >= (use == rn::kArpIsAt ? 42u : 78u) && slot >= len;
            out_len = rn::build(CheckedMem{fa, fend, da, da + (ok ? len : 0u)}, fa, flen, use, e, da, slot);
            if (out_len != (ok ? len : 0u)) {
                fprintf(stderr, "length %u where %u is due\n", out_len, ok ? len : 0u);
                exit(3);
            }
        }
        const uint32_t res[2] = {code, out_len};
        fwrite(res, 4, 2, out);
        fwrite(u, 4, 6, out);
        fwrite(region, 1, sizeof region, out);
    }
    fclose(out);
    return 0;
}
