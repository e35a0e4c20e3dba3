// wc_k_rxecho.hip -- the RX echo kernel on gfx950: the delivered datagrams of
// the sockets that are switched on become a TX batch for wc_tx_pump -- inetd's
// port 7 (inetd.c:161-169), which hands every received iov back to w_tx with
// the address, port and TOS udp_rx left in it.  DESIGN.md section 4.15.  The
// map from entry to frame, the classification, the descriptor and destination
// words and the copy's addressing are wc_rx_echo.h's.
//
// k_rx_echo, ONE launch for every n and m, one wave per workgroup, lane l =
// entry 64 b + l:
//   1. every workgroup reads d_start's first ns + 1 entries and d_map (2.5 KB,
//      L2-hot after the first), and scans the lengths of the switched-on runs
//      in LDS (re::run_len, eight re::scan_step rounds of four elements per
//      lane): no compaction pass, no workgroup waits for another;
//   2. each lane finds its entry's socket and list position by re::where_of's
//      eight halvings, reads the list entry, the record (one 16-byte load) and
//      the frame's offset and length, classifies (re::classify), and for an
//      ECHO entry reads the source address and the Ethernet source as the
//      aligned dwords that hold them (rr::frame_dword);
//   3. desc goes out as one 8-byte store per lane, af / status / src / tx_off
//      one element per lane -- consecutive lanes, consecutive addresses; the 24
//      bytes of a destination are transposed through LDS so that each of the
//      six store instructions writes 256 consecutive bytes (the LDS writes at
//      a stride of six dwords are 2-way bank conflicts, 384 dwords per wave:
//      left as they are);
//   4. copy mode: sixteen rounds, in each of which the wave's four 16-lane
//      groups move four entries' payloads (re::copy_lane): a lane has up to six
//      16-byte destination chunks' source loads in flight before its first
//      store, so four MTU payloads are in flight per wave.  The grid is m / 64
//      waves -- at most 1024, one per SIMD -- so occupancy cannot hide latency
//      here and the loads in flight per wave must: section 4.15.
// Stores are plain vector stores: aligned chunks and dwords inside the payload,
// 2-byte / byte stores at its two ends, so a neighbouring slot that shares a
// dword, a chunk or a cache line keeps every byte of its own.  Reads of frame
// bytes are aligned dwords / chunks that overlap the bytes wanted, all inside
// the aligned 16-byte chunks that overlap the frame.  The only atomic is
// *skipped's, one per wave with a skipped entry; *count is written by
// workgroup 0 alone.  The same input gives the same output.
// Roofline: HBM in copy mode (payload read once, written once); launch and
// dependent-load latency otherwise (start -> list -> record -> frame).
#include "wc_device.h"
#include "wc_rx_echo.h"

namespace wc {
namespace {

typedef u32x4 __attribute__((address_space(1))) *gst128e_ptr;
typedef uint64_t __attribute__((address_space(1))) *gst64e_ptr;

struct EchoMem : GlobalMem { // and re::copy_lane's accesses on rr::Quad
    __device__ __forceinline__ rr::Quad ld128(uint64_t a) const
    {
        const u32x4 v = load_chunk<false>(a);
        return rr::Quad{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void st128(uint64_t a, const rr::Quad &q) const
    {
        *(gst128e_ptr)(uintptr_t)a = u32x4{q.x, q.y, q.z, q.w};
    }
};

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return lo | ((uint64_t)hi << 32);
}

__global__ void __launch_bounds__(re::kWave) k_rx_echo(const RxEchoArgs a)
{
    __shared__ uint64_t S[2][re::kRuns];
    __shared__ uint32_t T[6 * re::kWave];
    const uint32_t lane = threadIdx.x;
    const bool rx = a.n != 0 && a.ns != 0;
    const bool copy = a.tx_off == nullptr;

    // 1. the inclusive totals of the switched-on runs
#pragma unroll
    for (uint32_t k = 0; k < re::kRuns / re::kWave; ++k) {
        const uint32_t t = lane + re::kWave * k;
        uint64_t len = 0;
        if (rx && t < a.ns)
            len = re::run_len(a.start[t], a.start[t + 1], a.n, a.map[t]);
        S[0][t] = len;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < re::kScanSteps; ++s) {
#pragma unroll
        for (uint32_t k = 0; k < re::kRuns / re::kWave; ++k)
            re::scan_step(S[s & 1u], S[(s + 1u) & 1u], lane + re::kWave * k, 1u << s);
        __syncthreads();
    }
    static_assert(re::kScanSteps % 2u == 0u, "the totals end in S[0]");
    const uint64_t *inc = S[0];
    const uint64_t E = inc[re::kRuns - 1u];
    if (blockIdx.x == 0 && lane == 0)
        *a.count = E;
    if (a.m == 0)
        return;

    // 2. this lane's entry
    const uint32_t j = blockIdx.x * re::kWave + lane;
    const bool inm = j < a.m;
    const bool live = inm && j < E;
    uint32_t st = re::kNone, sock = 0, flen = 0, from = 0xFFFFFFFFu;
    uint64_t off = 0;
    re::Rec r = re::rec_of(0u, 0u, 0u, 0u);
    if (live) {
        const re::Where w = re::where_of(inc, a.ns, j);
        sock = a.map[w.s];
        const uint64_t idx = a.list[a.start[w.s] + w.pos];
        const bool in = idx < a.n;
        if (in) {
            const u32x4 q = load_chunk<false>((uint64_t)(uintptr_t)a.rec + 16ull * idx);
            r = re::rec_of(q.x, q.y, q.z, q.w);
            off = a.offs[idx];
            flen = a.flens[idx];
            from = (uint32_t)idx;
        }
        st = re::classify(in, r, flen, copy, a.out_slot_bytes);
    }
    const bool echo = st == re::kEcho;
    const uint32_t h = re::hl_tx(r.af);
    const uint64_t fa = (uint64_t)(uintptr_t)a.base + off;
    uint32_t d[2], t[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (echo) {
        const GlobalMem gm{};
        const uint64_t fend = fa + flen;
        uint32_t src[4] = {rr::frame_dword(gm, fa, fend, r.src_off), 0u, 0u, 0u};
        if (r.af == 6u) {
            src[1] = rr::frame_dword(gm, fa, fend, r.src_off + 4u);
            src[2] = rr::frame_dword(gm, fa, fend, r.src_off + 8u);
            src[3] = rr::frame_dword(gm, fa, fend, r.src_off + 12u);
        }
        const uint32_t mac0 = rr::frame_dword(gm, fa, fend, 6u);
        const uint32_t mac1 = rr::frame_dword(gm, fa, fend, 10u);
        re::desc_words(r, a.ip_id ? (uint32_t)a.ip_id[j] : 0u, sock, j, d);
        re::dst_words(r, src, mac0, mac1, t);
    } else {
        re::inert_words(j, d);
    }

    // 3. the metadata
    if (inm) {
        *(gst64e_ptr)(uintptr_t)(a.desc + 2ull * j) = d[0] | ((uint64_t)d[1] << 32);
        a.af[j] = (uint8_t)(echo ? r.af : 0u);
        a.status[j] = (uint8_t)st;
        if (a.src)
            a.src[j] = from;
        if (a.tx_off)
            a.tx_off[j] = echo ? off + (r.hl - h) : 0ull;
    }
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k)
        T[6u * lane + k] = t[k];
    __syncthreads();
    const uint64_t w0 = 6ull * re::kWave * blockIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) {
        const uint32_t w = re::kWave * k + lane;
        if (w0 + w < 6ull * a.m)
            a.dsts[w0 + w] = T[w];
    }
    const uint64_t skips = __ballot(inm && re::is_skip(st));
    if (a.skipped && skips && lane == 0)
        atomicAdd((unsigned long long *)a.skipped, (unsigned long long)__popcll(skips));

    // 4. the payloads
    if (!copy)
        return;
    const uint32_t len = echo ? r.data_len : 0u;
    const uint64_t sa = fa + r.data_off;
    const uint64_t dd = (uint64_t)(uintptr_t)a.out_base + (echo ? a.out_off[j] : 0ull) + 14u + h + 8u;
    const EchoMem mem{};
    const uint32_t g = lane & (re::kGroup - 1u);
    for (uint32_t rd = 0; rd < re::kWave; rd += re::kWave / re::kGroup) {
        const int e = (int)(rd + lane / re::kGroup);
        const uint32_t len_e = (uint32_t)__shfl((int)len, e);
        const uint64_t sa_e = shfl_u64(sa, e), dd_e = shfl_u64(dd, e);
        if (len_e != 0u)
            re::copy_lane(mem, sa_e, dd_e, len_e, g);
    }
}

} // namespace

hipError_t launch_rx_echo(const RxEchoArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_rx_echo, dim3(re::grid_of(a.m)), dim3(re::kWave), 0, st, a);
    return hipGetLastError();
}

} // namespace wc
