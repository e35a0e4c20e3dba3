// wc_rx_answer.h -- what the RX answer's frames launch (wc_k_rxanswer.hip,
// k_rx_answer_frames), its launcher and a host test share, each stated once
// (DESIGN.md section 4.14): how one grid of 256-thread workgroups is split
// between the three roles -- the reply build (one wave per reply), the
// neighbour build and the update records (one lane per entry each) -- and
// which role and rank a workgroup has.  Plain C++ (no device builtin), so the
// kernel and a host program compile the same lines.
#pragma once

#include <stdint.h>

#include "wc_tx_build.h" // WC_HD

namespace wc {
namespace ra {

constexpr uint32_t kSmall = 4096u;   // WC_RX_ANSWER_SMALL
constexpr uint32_t kSmallApply = 1024u; // WC_RX_ANSWER_SMALL_APPLY: u_m where a table is given
constexpr uint32_t kThreads = 256u;  // a workgroup of the frames launch
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kReplyPer = kWaves;   // replies a workgroup takes per step
constexpr uint32_t kLanePer = kThreads;  // entries a lane role's workgroup takes per step

enum : uint32_t { kRoleReply = 0, kRoleNeigh = 1, kRoleUpdate = 2 };

// The workgroups of the three roles, in this order in the grid.
struct Split {
    uint32_t gr, gn, gu;
};

// The most workgroups a grid may have on a device of `cus` compute units that
// each hold `per_cu` of them at once -- and never fewer than three: no
// workgroup has two roles, so three lists with an entry each need three.
WC_HD uint32_t grid_cap(uint32_t cus, uint32_t per_cu)
{
    const uint64_t c = (uint64_t)cus * per_cu;
    return c < 3u ? 3u : c > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)c;
}

WC_HD uint32_t blocks_for(uint32_t m, uint32_t per)
{
    return m / per + (m % per != 0u);
}

// Each role is sized by its m; where the sum is more than cap (>= 3) allows,
// the two lane roles -- at most sixteen workgroups each on the small path --
// keep up to a quarter of it each and the reply role strides over the rest.
// A role with m = 0 has no workgroup, one with m > 0 at least one.
WC_HD Split split(uint32_t r_m, uint32_t n_m, uint32_t u_m, uint32_t cap)
{
    const uint32_t quarter = cap / 4u ? cap / 4u : 1u;
    Split s;
    s.gn = blocks_for(n_m, kLanePer);
    s.gu = blocks_for(u_m, kLanePer);
    s.gr = blocks_for(r_m, kReplyPer);
    s.gn = s.gn < quarter ? s.gn : quarter;
    s.gu = s.gu < quarter ? s.gu : quarter;
    const uint32_t rest = cap - s.gn - s.gu; // >= 1: two quarters, or 1 + 1 of 3
    s.gr = s.gr < rest ? s.gr : rest;
    return s;
}

WC_HD uint32_t grid_of(const Split &s)
{
    return s.gr + s.gn + s.gu;
}

// Workgroup b < grid_of(s): its role, the first workgroup of that role and
// how many the role has -- the role's entries are strided by (b - first) and
// count.
struct Role {
    uint32_t kind, first, count;
};

WC_HD Role role_of(const Split &s, uint32_t b)
{
    if (b < s.gr)
        return Role{kRoleReply, 0u, s.gr};
    if (b < s.gr + s.gn)
        return Role{kRoleNeigh, s.gr, s.gn};
    return Role{kRoleUpdate, s.gr + s.gn, s.gu};
}

// The reply role: wave w of its workgroup `rank` starts at first_reply and
// steps by reply_step.  The lane roles: thread t starts at first_entry and
// steps by entry_step.
WC_HD uint64_t first_reply(uint32_t rank, uint32_t w) { return (uint64_t)rank * kReplyPer + w; }
WC_HD uint64_t reply_step(uint32_t count) { return (uint64_t)count * kReplyPer; }
WC_HD uint64_t first_entry(uint32_t rank, uint32_t t) { return (uint64_t)rank * kLanePer + t; }
WC_HD uint64_t entry_step(uint32_t count) { return (uint64_t)count * kLanePer; }

// The apply launch: one workgroup of kApplyThreads threads; wave w takes the
// entries from 256 w on, 64 at a time, so kApplySteps steps reach kSmall.
constexpr uint32_t kApplyThreads = 1024u, kApplyWaves = kApplyThreads / 64u;
constexpr uint32_t kApplySteps = kSmall / kApplyThreads;
static_assert(kApplySteps * kApplyThreads == kSmall, "one workgroup's reach");

WC_HD uint32_t apply_index(uint32_t wave, uint32_t step, uint32_t lane)
{
    return wave * (64u * kApplySteps) + 64u * step + lane;
}

} // namespace ra
} // namespace wc
