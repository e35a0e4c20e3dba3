// wc_rx_demux.h -- what the RX demultiplex kernels (wc_k_rxdemux.hip) and the
// RX drain kernels (wc_k_rxdrain.hip) share on the device, each stated once:
// the block geometry (sixteen waves, four 64-frame steps each, so that (wave,
// step, lane) order is ring order), the class ranking of a wave's lanes by
// ballots (class_peers, class_rank), and the socket id of one frame from its
// record and its address bytes (window_bytes, frame_sock).  The table's layout,
// hash and probe are wc_rx_socktab.h's.
#pragma once

#include "wc_device.h"
#include "wc_rx_socktab.h"

namespace wc {
namespace {

constexpr int kDmxThreads = 1024;
constexpr int kDmxWaves = kDmxThreads / 64;
constexpr int kDmxSteps = 4;                                  // 64-frame steps per wave
constexpr uint32_t kDmxWaveFrames = 64u * kDmxSteps;          // 256
constexpr uint32_t kDmxBlock = kDmxWaveFrames * kDmxWaves;    // 4096 frames per block
constexpr uint32_t kSockNone = 0xFEu, kSockUnbound = 0xFFu;   // WC_RX_SOCK_*
constexpr uint32_t kDmxStarts = 256;

// The lanes of this wave whose id equals this lane's, among those with
// `counted` (0 for a lane without it).  Every lane of the wave calls it.
__device__ __forceinline__ uint64_t class_peers(uint32_t id, bool counted)
{
    uint64_t m = __ballot(counted);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (id >> b) & 1u;
        const uint64_t set = __ballot(bit);
        m &= bit ? set : ~set;
    }
    return counted ? m : 0ull;
}

__device__ __forceinline__ bool class_counted(uint32_t id, uint32_t ns)
{
    return id < ns || id == kSockUnbound;
}

// One step of a wave's ranking: this lane's rank among the lanes of its class
// so far in the wave (run[id] before the step plus the peers below it), and
// the class's running count moved on by one lane.  run: this wave's 256
// counters in LDS; the wave's own LDS operations execute in order.
__device__ __forceinline__ uint32_t class_rank(uint32_t *run, uint32_t id, bool counted)
{
    const uint64_t peers = class_peers(id, counted);
    const uint32_t below = mbcnt64(peers);
    uint32_t r = 0;
    if (counted)
        r = run[id] + below;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (counted && below == 0u)
        run[id] = r + (uint32_t)__builtin_popcountll(peers);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return r;
}

// Bytes [s, s + 32) of the 48-byte window w[0 .. 12) as eight dwords (s < 16).
__device__ __forceinline__ void window_bytes(uint32_t w[13], uint32_t s, uint32_t d[8])
{
    w[12] = 0u;
    if (s & 4u) {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            w[k] = w[k + 1];
    }
    if (s & 8u) {
#pragma unroll
        for (int k = 0; k < 11; ++k)
            w[k] = w[k + 2];
    }
    const uint32_t sh = 8u * (s & 3u);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        d[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> sh);
}

// The socket id of the frame at `frame` with record words r (af != 0): both
// addresses through the aligned chunks that overlap them -- `last` is the
// chunk of their last byte, never passed, so an IPv4 frame's loads end with
// its destination address --, then the table's two-step lookup.
__device__ __forceinline__ uint32_t frame_sock(uint64_t frame, const u32x4 &r,
                                               const uint32_t *slots, uint32_t nslots)
{
    const uint32_t af = r.z & 0xFFu;
    const bool v4 = af == 4u;
    const uint64_t at = frame + (v4 ? 14u + 12u : 14u + 8u);
    const uint64_t first = at & ~15ull, last = (at + (v4 ? 7u : 31u)) & ~15ull;
    const u32x4 c0 = load_chunk<false>(first);
    const u32x4 c1 = load_chunk<false>(first + 16u < last ? first + 16u : last);
    const u32x4 c2 = load_chunk<false>(last);
    uint32_t w[13] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, 0u};
    uint32_t d[8];
    window_bytes(w, (uint32_t)(at & 15u), d);
    // IPv4: src, dst = d[0], d[1]; IPv6: src = d[0..3], dst = d[4..7]
    uint32_t l[4], rm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        l[j] = v4 ? d[1] : d[4 + j];
        rm[j] = d[j];
    }
    uint32_t k[tab::kTabKeyWords];
    tab::tab_key(k, af, 1u, r.y >> 16, r.y & 0xFFFFu, l, rm); // local = dport, remote = sport
    return tab::tab_lookup(slots, nslots, k);
}

// The same id where the caller holds both addresses already (the RX drain
// kernel: out of the frame's header chunks): src / dst as dwords in packet
// order, IPv4 in word 0.  tab_key drops the words an IPv4 key ignores.
__device__ __forceinline__ uint32_t addr_sock(const u32x4 &r, const uint32_t (&src)[4],
                                              const uint32_t (&dst)[4], const uint32_t *slots,
                                              uint32_t nslots)
{
    uint32_t k[tab::kTabKeyWords];
    tab::tab_key(k, r.z & 0xFFu, 1u, r.y >> 16, r.y & 0xFFFFu, dst, src);
    return tab::tab_lookup(slots, nslots, k);
}

} // namespace
} // namespace wc
