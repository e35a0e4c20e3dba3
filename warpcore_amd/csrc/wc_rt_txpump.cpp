// wc_rt_txpump.cpp -- TX pump (wc_tx_pump_scratch, wc_tx_pump): the argument
// checks -- the chain's own, through the functions its calls use --, the two
// launches (wc_k_txpump.hip's plan, wc_k_txbuild.hip's gated build) for a batch
// of at most WC_TX_PUMP_SMALL frames to at most WC_TX_PUMP_SMALL_DST
// destinations with at most as many solicitation slots, and for a larger one
// the three calls it stands for, one after another on the caller's stream
// through the one scratch, then the same gated build.

#include "wc_rt.h"
#include "wc_tx_pump.h"

#include <algorithm>

using namespace wc::rt;
namespace tn = wc::tn;
namespace tp = wc::tp;

static_assert(WC_TX_PUMP_SMALL == tp::kSmall && WC_TX_PUMP_SMALL_DST == tp::kSmallDst &&
                  WC_TX_PUMP_HELD == tp::kHeld,
              "header and kernels agree");
static_assert(WC_TX_PUMP_HELD > WC_TX_TRUNCATED, "not an enum wc_tx_status code");
static_assert(sizeof(struct wc_tx_pump_out) == 13 * sizeof(void *), "thirteen pointers");

extern "C" {

// The larger of what the chain's calls ask for (they run one after another on
// the stream and share it); the two launches of the small path use none, but
// ask for the same, so that the function never decreases.
uint64_t wc_tx_pump_scratch(uint64_t n, uint32_t ndst)
{
    if (ndst > tn::kResolveMax)
        return 0;
    return std::max(wc_tx_resolve_scratch(ndst), wc::rxsel_scratch_bytes(n));
}

int wc_tx_pump(const void *d_tab, struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
               const struct wc_tx_desc *d_desc, uint64_t n, const struct wc_tx_sock *d_socks,
               uint32_t ns, void *d_base, const uint64_t *d_off, uint32_t slot_bytes, uint32_t flags,
               const struct wc_rx_engine *d_eng, void *d_sol_base, const uint64_t *d_sol_off,
               uint32_t m, uint32_t sol_slot_bytes, const struct wc_tx_pump_out *out, void *d_scratch,
               void *stream)
{
    if (!out || n > kRxListMax || ns > WC_TX_BUILD_MAX_SOCKS || ndst > tn::kResolveMax)
        return WC_EINVAL;
    const struct wc_tx_pump_out &o = *out;
    if (!o.miss_count || !o.held_count || !o.sol_built)
        return WC_EINVAL;
    if (slot_bytes > 65535u || sol_slot_bytes > 65535u)
        return WC_EINVAL;
    if (flags & ~(uint32_t)WC_TX_ZERO_UDP_CKSUM) // (WC_TX_NO_STORE: the build's own)
        return WC_EINVAL;
    // each side's rules are its chain call's, a list always asked for
    if (ndst != 0 && (!tx_resolve_ptrs_ok(d_tab, d_dsts, d_af, o.state, d_scratch) || !o.miss_list))
        return WC_EINVAL;
    if (n != 0) {
        if (!tx_hold_ptrs_ok(d_desc, o.hold, d_socks, ns, o.state, d_af, ndst, true, d_scratch) ||
            !o.held_list)
            return WC_EINVAL;
        if (tx_build_args(d_base, d_off, d_desc, d_socks, ns, d_dsts, ndst, o.frame_len, o.status))
            return WC_EINVAL;
    }
    if (m != 0 && !o.sol_len)
        return WC_EINVAL;
    if (m != 0 && ndst != 0 &&
        !tx_solicit_ptrs_ok(d_dsts, d_af, o.miss_list, o.miss_count, d_eng, d_sol_base, d_sol_off))
        return WC_EINVAL;

    hipStream_t st = (hipStream_t)stream;
    Ready R;
    if (R.rc)
        return R.rc;
    const bool nt = R.C.nt != 0;
    // m too: more slots than the small path's destinations can ever fill are the
    // chain's to zero, with a grid, not one workgroup's
    const bool small =
        n <= WC_TX_PUMP_SMALL && ndst <= WC_TX_PUMP_SMALL_DST && m <= WC_TX_PUMP_SMALL_DST;
    if (small) { // (n = ndst = 0: the plan launch alone writes the zeros)
        const wc::TxPumpArrays a{o.state,     o.miss_list,  o.miss_count, o.hold,
                                 o.held_list, o.held_count, o.sol_len,    o.sol_built};
        const hipError_t e =
            wc::launch_tx_pump_plan(d_tab, d_dsts, d_af, ndst, d_desc, (uint32_t)n, d_socks, ns,
                                    d_eng, d_sol_base, d_sol_off, m, sol_slot_bytes, a, st);
        if (e != hipSuccess)
            return hip_err(e);
    } else {
        // an empty side: its count alone, whatever the other pointers are
        int rc = ndst != 0 ? wc_tx_resolve(d_tab, d_dsts, d_af, ndst, o.state, o.miss_list,
                                           o.miss_count, d_scratch, stream)
                           : rx_zero_counts(o.miss_count, nullptr, st);
        if (rc == WC_OK)
            rc = n != 0 ? wc_tx_hold_plan(d_desc, n, d_socks, ns, o.state, d_af, ndst, o.hold,
                                          o.held_list, o.held_count, d_scratch, stream)
                        : rx_zero_counts(o.held_count, nullptr, st);
        if (rc == WC_OK)
            rc = wc_tx_solicit_build(d_dsts, d_af, ndst, o.miss_list, o.miss_count, d_eng,
                                     d_sol_base, d_sol_off, m, sol_slot_bytes, o.sol_len,
                                     o.sol_built, stream);
        if (rc != WC_OK)
            return rc;
    }
    if (n == 0)
        return WC_OK;
    return hip_err(wc::launch_tx_build_gated(d_base, d_off, d_desc, n, d_socks, ns, d_dsts, ndst,
                                             slot_bytes, flags, o.hold, o.frame_len, o.status,
                                             o.out_ip_hdr, o.out_udp, o.errors, nt, st));
}

} // extern "C"
