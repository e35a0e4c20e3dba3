// wc_tx_pump.h -- what the TX pump's gated build (wc_k_txbuild.hip,
// k_tx_build_gated), its plan launch (wc_k_txpump.hip) and a host test share,
// each stated once: the per-frame gate that joins
// wc_tx_hold_plan's code to the build's check chain, and the plan launch's
// steps over one destination, which are wc_tx_neigh.h's own resolve_find /
// resolve_mark over a set, a where array and a copy of the state bytes that
// the caller places (the kernel: in LDS).  Plain C++ (no device builtin), so
// the kernels and a host program compile the same lines.
#pragma once

#include "wc_tx_neigh.h"

namespace wc {
namespace tp {

constexpr uint32_t kSmall = 4096u, kSmallDst = 4096u; // WC_TX_PUMP_SMALL, _SMALL_DST
constexpr uint32_t kHeld = 0x80u;                     // WC_TX_PUMP_HELD

// One frame of the gated build: hold = its wc_tx_hold_plan code, x = the
// build's check chain over the same descriptor and tables (the zero-UDP flag
// is already in x.status: txb::decide chose between the two sealed codes).
//   READY      the build's own result: status, length, built, its error.
//   MALFORMED  nothing built, WC_TX_MALFORMED, an error.
//   HELD       nothing built, kHeld, no error.
// Any other byte (the plan writes none) counts as MALFORMED.
struct Gate {
    uint32_t status, flen;
    bool built, error;
};

WC_HD Gate gate(uint32_t hold, const txb::Decide &x)
{
    Gate g;
    const bool ready = hold == tn::kThReady, held = hold == tn::kThHeld;
    g.built = ready && x.status <= txb::kSealedZeroUdp;
    g.status = held ? kHeld : !ready ? txb::kMalformed : x.status;
    g.flen = g.built ? x.flen : 0u;
    g.error = !g.built && !held;
    return g;
}

// The plan launch's destination steps.  set: 2 set_slots(ndst) zeroed words,
// where: ndst words, lstate: ndst bytes -- all the workgroup's own (Words
// reaches them and the tables through the same calls).  Between find and mark
// of any two destinations lies a barrier; within each step the destinations
// may run in any order.
template <class Words>
WC_HD void dst_find(const Words &w, const uint32_t *tab, uint32_t cap, uint32_t *dsts,
                    const uint8_t *afs, uint32_t ndst, uint32_t k, uint32_t *set, uint8_t *lstate,
                    uint32_t *where)
{
    tn::resolve_find(w, tab, cap, dsts, afs, ndst, k, set, tn::set_slots(ndst), lstate, where);
}

template <class Words>
WC_HD void dst_mark(const Words &w, uint32_t ndst, uint32_t k, const uint32_t *set, uint8_t *lstate,
                    const uint32_t *where)
{
    tn::resolve_mark(w, k, set, tn::set_slots(ndst), lstate, where);
}

} // namespace tp
} // namespace wc
