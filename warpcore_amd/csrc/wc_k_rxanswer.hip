// wc_k_rxanswer.hip -- the RX answer's two launches on gfx950: for at most
// ra::kSmall entries in each of the three lists an RX plan leaves, everything
// wc_rx_reply_build, wc_rx_neigh_updates, wc_rx_neigh_build and wc_neigh_apply
// leave, with no memset in front of either launch.
//
// k_rx_answer_frames: one grid of 256-thread workgroups.  A workgroup's role is
// a function of blockIdx.x alone (ra::role_of over the ra::Split the launcher
// computed), so the branch is uniform per workgroup and scalar:
//   the first gr   rx_reply_build_body, one wave per reply at a time;
//   the next  gn   rx_neigh_build_body, one lane per entry;
//   the last  gu   rx_neigh_updates_body, one lane per entry.
// The bodies are the three list kernels' own (wc_rx_build.h), over the role's
// share of the grid instead of a whole one, and without the built count: no
// role touches one, so there is no atomic and nothing has to be zeroed first.
// With n = 0 a role stores its zero lengths or zero records and reads nothing.
//
// k_rx_answer_apply: ONE workgroup of 1024 threads behind it on the stream
// (stream order is the only ordering between the two).  Wave w takes the
// entries from 256 w on, 64 at a time (k_rx_drain_lists' scheme):
//   A. the two built counts: the j < r_m with r_out_len[j] != 0, the j < n_m
//      with n_out_len[j] != 0 -- one ballot per step, the sixteen waves' totals
//      through LDS, one lane stores each 64-bit count (written, not added);
//   B. claim: record j < MIN(*ucount, u_m) runs tn::apply_claim on the table
//      where it lies; the entry index stays in LDS (16 KiB) instead of global
//      scratch; the dropped records are counted per wave;
//   C. commit: tn::apply_commit from the LDS index; the dropped total is added
//      to *dropped once, where it is given and not 0.
// A, B and C are separated by workgroup barriers; with tab NULL or u_m = 0, B
// and C are skipped.  apply_claim and apply_commit are wc_tx_neigh.h's,
// unchanged, so section 4.11's argument carries over: lanes tell each other
// nothing but through atomics on the table's own words, read back with
// agent-scope loads, and upd is immutable for the whole launch.
//
// In both kernels no workgroup waits for another, nothing spins, every loop is
// bounded by an m, by cap or by a slot length, and all global stores are plain
// vector stores or the table's existing atomics (and the one atomicAdd on
// *dropped, as wc_neigh_apply's).
// Roofline: latency -- a few dependent loads per entry; two barriers.
#include "wc_rx_build.h"

#include "wc_rx_answer.h"
#include "wc_tx_neigh.h"

namespace wc {
namespace {

static_assert(ra::kThreads == 256u && ra::kWaves == 4u, "the frames launch's workgroup");

__global__ void __launch_bounds__(ra::kThreads)
k_rx_answer_frames(const RxAnswerArgs a, const ra::Split s)
{
    const ra::Role role = ra::role_of(s, blockIdx.x);
    const uint32_t rank = blockIdx.x - role.first;
    if (role.kind == ra::kRoleReply) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const uint64_t j0 = ra::first_reply(rank, w), S = ra::reply_step(role.count);
        if (a.n == 0) { // no frame, no reply
            for (uint64_t j = j0; j < a.r_m; j += S)
                if ((threadIdx.x & 63u) == 0u)
                    a.r_out_len[j] = 0;
            return;
        }
        rx_reply_build_body<ra::kWaves, false>(
            a.base, a.offs, a.flens, a.n, a.action, a.rlist, (const unsigned long long *)a.rcount,
            a.eng, a.r_out_base, a.r_out_off, a.r_m, a.slot_bytes, a.ip_id, a.r_out_len, nullptr, j0,
            S);
    } else if (role.kind == ra::kRoleNeigh) {
        const uint64_t j0 = ra::first_entry(rank, threadIdx.x), S = ra::entry_step(role.count);
        if (a.n == 0) {
            for (uint64_t j = j0; j < a.n_m; j += S)
                a.n_out_len[j] = 0;
            return;
        }
        rx_neigh_build_body<ra::kWaves, false>(
            a.base, a.offs, a.flens, a.n, a.nact, a.nrlist, (const unsigned long long *)a.nrcount,
            a.eng, a.n_out_base, a.n_out_off, a.n_m, a.slot_bytes, a.n_out_len, nullptr, j0, S);
    } else {
        const uint64_t j0 = ra::first_entry(rank, threadIdx.x), S = ra::entry_step(role.count);
        if (a.n == 0) { // no frame, no record
            for (uint64_t j = j0; j < a.u_m; j += S) {
                uint32_t *o = a.upd + 6u * j;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    o[k] = 0u;
            }
            return;
        }
        rx_neigh_updates_body(a.base, a.offs, a.flens, a.n, a.nact, a.ulist,
                              (const unsigned long long *)a.ucount, a.u_m, a.upd, j0, S);
    }
}

constexpr int kRaThreads = (int)ra::kApplyThreads, kRaWaves = (int)ra::kApplyWaves;
constexpr int kRaSteps = (int)ra::kApplySteps; // four steps of 64 per wave
static_assert(tn::kUpdWords == 6u, "the record as six dwords");

// upd and the length arrays were written by the launch in front; nothing here
// writes them.  tab is read and written by every lane: no __restrict__.
__global__ void __launch_bounds__(kRaThreads)
k_rx_answer_apply(const uint16_t *__restrict__ r_out_len, uint32_t r_m,
                  const uint16_t *__restrict__ n_out_len, uint32_t n_m,
                  unsigned long long *__restrict__ r_built,
                  unsigned long long *__restrict__ n_built, uint32_t *tab,
                  const uint32_t *__restrict__ upd, const unsigned long long *__restrict__ ucount,
                  uint32_t u_m, unsigned long long *__restrict__ dropped)
{
    // (a lane reads back in C only the entries it wrote in B: four registers
    // would do, but an LDS array lets B and C stay rolled loops without a
    // per-step register array -- k_tx_pump_plan's choice for `where`)
    __shared__ uint32_t ent[ra::kSmall];
    __shared__ uint32_t wt[3][kRaWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DevWords w{};

    // A: this wave's built replies of either kind
    uint32_t nr = 0, nn = 0; // wave-uniform
#pragma unroll
    for (int step = 0; step < kRaSteps; ++step) {
        const uint32_t k = ra::apply_index((uint32_t)wave, (uint32_t)step, (uint32_t)lane);
        const bool r = k < r_m && r_out_len[k] != 0;
        const bool b = k < n_m && n_out_len[k] != 0;
        nr += (uint32_t)__builtin_popcountll(__ballot(r));
        nn += (uint32_t)__builtin_popcountll(__ballot(b));
    }
    if (lane == 0) {
        wt[0][wave] = nr;
        wt[1][wave] = nn;
    }
    __syncthreads();
    if (threadIdx.x < 2) { // thread 0: *r_built, thread 1: *n_built
        uint32_t all = 0;
#pragma unroll
        for (int v = 0; v < kRaWaves; ++v)
            all += wt[threadIdx.x][v];
        *(threadIdx.x == 0 ? r_built : n_built) = all;
    }
    if (!tab || u_m == 0) // (uniform: kernel arguments)
        return;

    // B: claim
    const uint32_t lim = (uint32_t)list_limit(ucount, u_m);
    const uint32_t cap = tn::tab_cap(w, tab);
    uint32_t ndrop = 0; // wave-uniform
#pragma unroll 1
    for (int step = 0; step < kRaSteps; ++step) {
        const uint32_t k = ra::apply_index((uint32_t)wave, (uint32_t)step, (uint32_t)lane);
        bool drop = false;
        if (k < lim)
            ent[k] = tn::apply_claim(w, tab, cap, upd, lim, k, drop);
        ndrop += (uint32_t)__builtin_popcountll(__ballot(drop));
    }
    if (lane == 0)
        wt[2][wave] = ndrop;
    // apply_claim's atomicMax on an entry's `last` returns nothing, so a lane
    // does not wait for it; a commit lane must not read `last` before every
    // claim lane's maximum has reached the memory the agent-scope load reads.
    // A workgroup barrier alone orders the workgroup's own scope, not device-
    // scope atomics still in flight: the agent-scope fence in front of it does
    // (each wave waits for its own outstanding atomics before it arrives).
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __syncthreads();

    // C: commit
#pragma unroll 1
    for (int step = 0; step < kRaSteps; ++step) {
        const uint32_t k = ra::apply_index((uint32_t)wave, (uint32_t)step, (uint32_t)lane);
        if (k < lim)
            tn::apply_commit(w, tab, cap, upd, k, ent[k]);
    }
    if (threadIdx.x == 0 && dropped) {
        uint32_t all = 0;
#pragma unroll
        for (int v = 0; v < kRaWaves; ++v)
            all += wt[2][v];
        if (all)
            atomicAdd(dropped, (unsigned long long)all);
    }
}

} // namespace

hipError_t launch_rx_answer_frames(const RxAnswerArgs &a, int cus, hipStream_t st)
{
    if (a.r_m > ra::kSmall || a.n_m > ra::kSmall || a.u_m > ra::kSmall)
        return hipErrorInvalidValue;
    // (one occupancy query per process, on the device current at the first call, as
    // list_grid's: a node's GPUs are alike; `cus` is the calling device's own)
    static const int per_cu = [] {
        int k = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, k_rx_answer_frames, (int)ra::kThreads,
                                                         0) != hipSuccess ||
            k < 1)
            k = 1;
        return k;
    }();
    const uint32_t cap = cus > 0 ? ra::grid_cap((uint32_t)cus, (uint32_t)per_cu)
                                 : (uint32_t)kMaxGridBlocks;
    const ra::Split s = ra::split(a.r_m, a.n_m, a.u_m, cap);
    const uint32_t grid = ra::grid_of(s);
    if (grid == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_rx_answer_frames, dim3(grid), dim3(ra::kThreads), 0, st, a, s);
    return hipGetLastError();
}

hipError_t launch_rx_answer_apply(const RxAnswerArgs &a, hipStream_t st)
{
    if (a.r_m > ra::kSmall || a.n_m > ra::kSmall || a.u_m > ra::kSmall)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rx_answer_apply, dim3(1), dim3(kRaThreads), 0, st,
                       (const uint16_t *)a.r_out_len, a.r_m, (const uint16_t *)a.n_out_len, a.n_m,
                       (unsigned long long *)a.r_built, (unsigned long long *)a.n_built, a.tab,
                       (const uint32_t *)a.upd, (const unsigned long long *)a.ucount, a.u_m,
                       (unsigned long long *)a.dropped);
    return hipGetLastError();
}

} // namespace wc
