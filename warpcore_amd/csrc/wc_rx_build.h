// wc_rx_build.h -- the loop bodies of the three RX list kernels, each stated
// once: k_rx_reply_build (wc_k_rxreply.hip), k_rx_neigh_updates and
// k_rx_neigh_build (wc_k_rxneigh.hip) instantiate them over a whole grid, and
// k_rx_answer_frames (wc_k_rxanswer.hip) over one role's workgroups of a shared
// grid (DESIGN.md sections 4.9, 4.10, 4.14).  What each body does, which bytes
// it may read and how it stores is said at the head of the kernel files; the
// parameters the two callers differ in:
//   WAVES    waves per workgroup (the built count's LDS words);
//   COUNT    whether the role's built total is added to *built, one atomic per
//            workgroup (block_count_add) -- the answer counts the stored
//            lengths in its second launch instead and passes built = nullptr;
//   j0, S    the first entry of this wave (reply build) or lane (the other
//            two) and its step: the role's first workgroup and workgroup count
//            as the caller's grid has them.
#pragma once

#include "wc_rx_hdr.h"
#include "wc_rx_neigh.h"
#include "wc_rx_reply.h"

namespace wc {
namespace {

typedef u32x4 __attribute__((address_space(1))) *gst128_ptr;

struct ReplyMem : GlobalMem { // and rr::copy_chunk's accesses on rr::Quad
    __device__ __forceinline__ rr::Quad ld128(uint64_t a) const
    {
        const u32x4 v = load_chunk<false>(a);
        return rr::Quad{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void st128(uint64_t a, const rr::Quad &q) const
    {
        *(gst128_ptr)(uintptr_t)a = u32x4{q.x, q.y, q.z, q.w};
    }
};

// One wave per reply at a time.  j0 and S are wave-uniform.
template <uint32_t WAVES, bool COUNT>
__device__ __forceinline__ void
rx_reply_build_body(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                    const uint16_t *__restrict__ flens, uint64_t n,
                    const uint8_t *__restrict__ action, const uint32_t *__restrict__ list,
                    const unsigned long long *__restrict__ count, const uint32_t *__restrict__ eng,
                    uint8_t *out_base, const uint64_t *__restrict__ out_off, uint32_t m,
                    uint32_t slot_bytes, const uint16_t *__restrict__ ip_id,
                    uint16_t *__restrict__ out_len, unsigned long long *__restrict__ built,
                    uint64_t j0, uint64_t S)
{
    const int lane = threadIdx.x & 63;
    const uint64_t lim = list_limit(count, m);
    const uint32_t mtu = rr::eng_mtu(eng);
    const ReplyMem mem{};
    uint32_t nbuilt = 0; // wave-uniform

    // A wave's replies are j, j + S, ...; each costs two dependent load rounds
    // in front of its stores (the frame's length fields; then its addresses and
    // data), because the two rounds in front of those -- the list entry, then
    // what it names -- are issued one and two replies ahead, beside the loads
    // of the reply being built.
    uint64_t j = j0;
    // (the slot and ip->id of reply j are read one reply ahead too)
    auto slot_of = [&](uint64_t k) { return k < m ? out_off[k] : 0u; };
    auto ipid_of = [&](uint64_t k) { return ip_id && k < m ? (uint32_t)ip_id[k] : 0u; };
    ListMeta cur = list_meta(list_entry(list, j, lim), n, action, offs, flens);
    uint64_t ooff = slot_of(j);
    uint32_t ipid = ipid_of(j);
    uint64_t idx_n = list_entry(list, j + S, lim);
    for (; j < m; j += S) {
        const ListMeta nxt = list_meta(idx_n, n, action, offs, flens);
        const uint64_t ooff_n = slot_of(j + S);
        const uint32_t ipid_n = ipid_of(j + S);
        idx_n = list_entry(list, j + 2 * S, lim);
        uint32_t len = 0;
        if (cur.live && rr::is_reply(cur.act)) { // (wave-uniform branches throughout)
            const uint32_t act = cur.act, flen = cur.flen;
            const uint64_t fa = (uint64_t)(uintptr_t)base + cur.off;
            const uint64_t fend = fa + flen;
            // vhl, tos, ip->len (IPv4) and ip6->len: frame bytes 14..17, 18..19
            const uint32_t g0 = rr::frame_dword(mem, fa, fend, 14u);
            const uint32_t g1 = rr::frame_dword(mem, fa, fend, 18u);
            const bool v4 = rr::reply_v4(act);
            const uint32_t hl = v4 ? ((g0 & 15u) * 4u) : 40u;
            const uint32_t ip_len = txb::bswap16(v4 ? g0 >> 16 : g1);
            const rr::Reply r = rr::reply_of(act, hl, ip_len, flen, mtu, slot_bytes);
            if (rr::is_reply(r.action)) {
                const rr::Req q = rr::request_of(mem, fa, fend, act, hl);
                const uint64_t da = (uint64_t)(uintptr_t)out_base + ooff;
                const uint64_t dd = da + (v4 ? 42u : 62u), sa = fa + r.s0;
                const uint32_t nd = rr::copy_dwords(dd, r.dlen);
                const rr::Chunks ch = rr::copy_chunks(dd, r.dlen);
                uint32_t acc = 0;
                for (uint32_t c = ch.c0 + (uint32_t)lane; c < ch.c1; c += 64u)
                    acc += rr::copy_chunk(mem, sa, dd, c);
                // the dwords in front of and behind the whole chunks: at most 4 + 4
                const uint32_t i = (uint32_t)lane < ch.i0 ? (uint32_t)lane
                                                          : ch.i1 + ((uint32_t)lane - ch.i0);
                if (i < nd)
                    acc += rr::copy_dword(mem, sa, dd, r.dlen, i);
                const uint32_t data = rr::fold16(group_sum<64>(acc));
                uint32_t h[16];
                rr::headers(r, q, eng, ipid, data, h);
                if (lane == 0)
                    txb::store_headers(mem, da, v4, h);
                len = r.len;
            }
        }
        if (lane == 0)
            out_len[j] = (uint16_t)len;
        nbuilt += len != 0u;
        cur = nxt;
        ooff = ooff_n;
        ipid = ipid_n;
    }
    if constexpr (COUNT)
        block_count_add<WAVES>(nbuilt, built);
}

// One lane per record.
__device__ __forceinline__ void
rx_neigh_updates_body(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                      const uint16_t *__restrict__ flens, uint64_t n,
                      const uint8_t *__restrict__ nact, const uint32_t *__restrict__ list,
                      const unsigned long long *__restrict__ count, uint32_t m,
                      uint32_t *__restrict__ upd, uint64_t j0, uint64_t S)
{
    const uint64_t lim = list_limit(count, m);
    const GlobalMem mem{};
    uint64_t j = j0;
    ListMeta cur = list_meta(list_entry(list, j, lim), n, nact, offs, flens);
    uint64_t idx_n = list_entry(list, j + S, lim);
    for (; j < m; j += S) {
        const ListMeta nxt = list_meta(idx_n, n, nact, offs, flens);
        idx_n = list_entry(list, j + 2 * S, lim);
        uint32_t u[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (cur.live && rn::is_update(cur.act))
            rn::record_of(mem, (uint64_t)(uintptr_t)base + cur.off, cur.flen, cur.act, u);
        uint32_t *o = upd + 6u * j;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            o[k] = u[k];
        cur = nxt;
    }
}

// One lane per reply.
template <uint32_t WAVES, bool COUNT>
__device__ __forceinline__ void
rx_neigh_build_body(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                    const uint16_t *__restrict__ flens, uint64_t n,
                    const uint8_t *__restrict__ nact, const uint32_t *__restrict__ list,
                    const unsigned long long *__restrict__ count, const uint32_t *__restrict__ eng,
                    uint8_t *out_base, const uint64_t *__restrict__ out_off, uint32_t m,
                    uint32_t slot_bytes, uint16_t *__restrict__ out_len,
                    unsigned long long *__restrict__ built, uint64_t j0, uint64_t S)
{
    const uint64_t lim = list_limit(count, m);
    const GlobalMem mem{};
    uint32_t nbuilt = 0;
    uint64_t j = j0;
    ListMeta cur = list_meta(list_entry(list, j, lim), n, nact, offs, flens);
    uint64_t ooff = j < m ? out_off[j] : 0u;
    uint64_t idx_n = list_entry(list, j + S, lim);
    for (; j < m; j += S) {
        const ListMeta nxt = list_meta(idx_n, n, nact, offs, flens);
        const uint64_t ooff_n = j + S < m ? out_off[j + S] : 0u;
        idx_n = list_entry(list, j + 2 * S, lim);
        uint32_t len = 0;
        if (cur.live && rn::is_reply(cur.act))
            len = rn::build(mem, (uint64_t)(uintptr_t)base + cur.off, cur.flen, cur.act, eng,
                            (uint64_t)(uintptr_t)out_base + ooff, slot_bytes);
        out_len[j] = (uint16_t)len;
        nbuilt += len != 0u;
        cur = nxt;
        ooff = ooff_n;
    }
    if constexpr (COUNT)
        block_count_add<WAVES>(group_sum<64>(nbuilt), built);
}

} // namespace
} // namespace wc
