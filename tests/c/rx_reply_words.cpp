// rx_reply_words.cpp -- the RX replies' shared statement (warpcore_amd/csrc/
// wc_rx_reply.h: filters, decision chain, reply lengths, header dwords, the
// data copy with its sum) compiled for the host alone and driven from a case
// file, so the lines the gfx950 kernels compile are held against
// tests/rx_reply_model.py without a GPU (tests/test_rx_reply_words.py).
//
// Input, per case (little-endian): the 844 table bytes, then uint32 verdict,
// sock (0x100: no d_sock), slot_bytes, action (0xFFFFFFFF: the plan's own),
// ip_id, source phase, destination phase, flen, then flen frame bytes.
// Output, per case: uint32 action, reply_len, out_len, then a 2304-byte region
// pre-filled with 0xA5 in which the reply starts at byte 16 + destination
// phase.  Every access is checked (checked_mem.h): loads aligned and overlapping the
// frame, stores naturally aligned and inside the reply.
#include "checked_mem.h"
#include "wc_rx_reply.h"

namespace rr = wc::rr;
namespace txb = wc::txb;

// in_cksum.c:107-137 on its own
static uint32_t oc16(const uint8_t *d, uint32_t n)
{
    uint32_t s = 0;
    for (uint32_t i = 0; i + 1 < n; i += 2)
        s += d[i] | (d[i + 1] << 8);
    if (n & 1u)
        s += d[n - 1];
    return s;
}

static uint32_t reduce(uint32_t s)
{
    while (s >> 16)
        s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out)
        return 2;
    alignas(16) static uint8_t src[4096], region[2304];
    for (;;) {
        uint32_t e[rr::kEngineWords], arg[8];
        if (fread(e, 4, rr::kEngineWords, in) != rr::kEngineWords)
            break;
        if (fread(arg, 4, 8, in) != 8)
            return 2;
        const uint32_t verdict = arg[0], sock = arg[1], slot = arg[2], force = arg[3], ip_id = arg[4],
                       sp = arg[5], dp = arg[6], flen = arg[7];
        if (flen > 2048 || sp > 15 || dp > 15 || slot > 2048)
            return 2;
        memset(src, 0x5A, sizeof src);
        uint8_t *fr = src + 16 + sp;
        if (fread(fr, 1, flen, in) != flen)
            return 2;
        uint8_t z[2048 + 64] = {}; // the frame alone, zeros behind it: what the chain may look at
        memcpy(z, fr, flen);
        const uint32_t mtu = rr::eng_mtu(e);

        // the plan, as k_rx_reply_plan feeds the chain
        rr::Frame f;
        f.verdict = verdict, f.flen = flen;
        f.unbound = sock == rr::kSockUnbound;
        f.v4 = z[12] == 0x08 && z[13] == 0x00;
        f.hl = f.v4 ? (z[14] & 15u) * 4u : 40u;
        f.proto = f.v4 ? z[23] : z[20];
        f.ip_len = f.v4 ? (z[16] << 8) | z[17] : (z[18] << 8) | z[19];
        uint32_t s[4], d[4];
        for (int k = 0; k < 4; ++k) {
            s[k] = le32(z + (f.v4 ? 26 : 22) + 4 * k);
            d[k] = le32(z + (f.v4 ? 30 : 38) + 4 * k);
        }
        f.mac_ok = rr::mac_ok(e, le32(z), le32(z + 4));
        const rr::Match am = rr::addr_match(e, f.v4, d, s);
        f.dst_ok = am.dst, f.src_ok = am.src;
        uint32_t sum_len;
        rr::Reply r = rr::chain_head(f, mtu, slot, sum_len);
        if (r.action == rr::kSum4) {
            const uint8_t *m = z + 14 + f.hl;
            r = rr::chain_tail(rr::kSum4, f, reduce(oc16(m, sum_len)), m[0], mtu, slot);
        } else if (r.action == rr::kSum6) {
            const uint8_t *ip = z + 14; // payload_cksum(ip, sum_len), in_cksum.c:155-164
            const uint32_t S = ((uint32_t)ip[6] << 24) + oc16(ip + 8, 32) + oc16(ip + 4, 2) +
                               oc16(ip + 40, sum_len - 40);
            r = rr::chain_tail(rr::kSum6, f, reduce(S), z[54], mtu, slot);
        }
        const uint32_t action = r.action, reply_len = r.len;

        // the build, as k_rx_reply_build runs it on the action byte it is handed
        memset(region, 0xA5, sizeof region);
        const uint32_t act = force != 0xFFFFFFFFu ? force : action;
        uint32_t out_len = 0;
        if (rr::is_reply(act)) {
            const uint64_t fa = (uint64_t)(uintptr_t)fr, fend = fa + flen;
            const uint64_t da = (uint64_t)(uintptr_t)region + 16u + dp;
            CheckedMem128<rr::Quad> mem{{fa, fend, da, da}};
            const uint32_t g0 = flen ? rr::frame_dword(mem, fa, fend, 14u) : 0u;
            const uint32_t g1 = flen ? rr::frame_dword(mem, fa, fend, 18u) : 0u;
            const bool v4 = rr::reply_v4(act);
            const uint32_t hl = v4 ? (g0 & 15u) * 4u : 40u;
            const uint32_t ipl = v4 ? txb::bswap16(g0 >> 16) : txb::bswap16(g1);
            const rr::Reply b = rr::reply_of(act, hl, ipl, flen, mtu, slot);
            if (rr::is_reply(b.action)) {
                mem.hi = da + b.len;
                const rr::Req q = rr::request_of(mem, fa, fend, act, hl);
                const uint64_t dd = da + (v4 ? 42u : 62u), sa = fa + b.s0;
                const uint32_t nd = rr::copy_dwords(dd, b.dlen);
                const rr::Chunks ch = rr::copy_chunks(dd, b.dlen);
                uint32_t acc = 0;
                for (uint32_t c = ch.c0; c < ch.c1; ++c)
                    acc += rr::copy_chunk(mem, sa, dd, c);
                for (uint32_t lane = 0; lane < 64; ++lane) { // the kernel's edge dwords
                    const uint32_t i = lane < ch.i0 ? lane : ch.i1 + (lane - ch.i0);
                    if (i < nd)
                        acc += rr::copy_dword(mem, sa, dd, b.dlen, i);
                }
                if (nd - (ch.i1 - ch.i0) > 64) {
                    fprintf(stderr, "more than 64 edge dwords\n");
                    exit(3);
                }
                uint32_t h[16];
                rr::headers(b, q, e, ip_id, rr::fold16(acc), h);
                txb::store_headers(mem, da, v4, h);
                out_len = b.len;
            }
        }
        const uint32_t res[3] = {action, reply_len, out_len};
        fwrite(res, 4, 3, out);
        fwrite(region, 1, sizeof region, out);
    }
    fclose(out);
    return 0;
}
