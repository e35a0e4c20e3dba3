// tx_build_words.cpp -- the TX build's shared statement (warpcore_amd/csrc/
// wc_tx_build.h: check chain, header dwords, phase stores) compiled for the
// host alone and driven from a case file, so the lines the gfx950 kernel and
// wc_tx_build_host compile are held against tests/tx_build_model.py without a
// GPU (tests/test_tx_build_words.py).
//
// Input, per case (little-endian): sock[52] dst[24] desc[8], then uint32
// sock_in, dst_in, slot_bytes, zero_udp, phase, paylen, then paylen payload
// bytes.  Output, per case: uint32 status, flen, ip_hdr, udp, then a 128-byte
// region pre-filled with 0xA5 in which the frame starts at byte 16 + phase.
// Every store is checked (checked_mem.h): natural alignment, inside the header
// bytes.
#include <vector>

#include "checked_mem.h"
#include "wc_tx_build.h"

namespace txb = wc::txb;

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out)
        return 2;
    alignas(16) uint8_t region[128];
    for (;;) {
        uint32_t w[txb::kSockWords], t[txb::kDstWords], dw[2], arg[6];
        if (fread(w, 4, txb::kSockWords, in) != txb::kSockWords)
            break;
        if (fread(t, 4, txb::kDstWords, in) != txb::kDstWords || fread(dw, 4, 2, in) != 2 ||
            fread(arg, 4, 6, in) != 6)
            return 2;
        std::vector<uint8_t> pay(arg[5] + 1);
        if (fread(pay.data(), 1, arg[5], in) != arg[5])
            return 2;
        const bool sock_in = arg[0], dst_in = arg[1], zero_udp = arg[3];
        const uint32_t phase = arg[4];
        if (!sock_in)
            memset(w, 0, sizeof w);
        if (!dst_in)
            memset(t, 0, sizeof t);
        const txb::Desc d = txb::desc_of(dw[0], dw[1]);
        const txb::Decide x = txb::decide(sock_in, w[0], dst_in, d.data_len, arg[2], zero_udp);
        const bool built = x.status <= txb::kSealedZeroUdp;
        // the payload's words from its first byte on, folded (in_cksum.c:107-120)
        uint32_t s = 0;
        if (built && !zero_udp) {
            if (arg[5] != d.data_len)
                return 2;
            for (uint32_t i = 0; i + 1 < arg[5]; i += 2)
                s += pay[i] | (pay[i + 1] << 8);
            if (arg[5] & 1u)
                s += pay[arg[5] - 1];
            s = (s & 0xFFFFu) + (s >> 16);
            s = (s & 0xFFFFu) + (s >> 16);
        }
        memset(region, 0xA5, sizeof region);
        uint32_t res[4] = {x.status, 0u, 0u, 0u};
        if (built) {
            const txb::Hdr h = txb::headers(x, d, w, t, s, zero_udp, true);
            const uint64_t fa = (uint64_t)(uintptr_t)region + 16u + phase;
            txb::store_headers(CheckedMem{0, 0, fa, fa + x.hb, "frame", "the headers"}, fa, x.v4,
                               h.h);
            res[1] = x.flen, res[2] = h.ip_hdr, res[3] = h.udp;
        }
        fwrite(res, 4, 4, out);
        fwrite(region, 1, sizeof region, out);
    }
    fclose(out);
    return 0;
}
