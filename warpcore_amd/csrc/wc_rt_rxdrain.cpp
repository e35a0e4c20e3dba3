// wc_rt_rxdrain.cpp -- RX drain (wc_rx_drain_scratch, wc_rx_drain): the
// argument checks, the two launches of wc_k_rxdrain.hip for a ring of at most
// WC_RX_DRAIN_SMALL frames, and for a larger one the four calls it stands for,
// one after another on the caller's stream through the one scratch (DESIGN.md
// section 4.12).

#include "wc_rt.h"
#include "wc_rx_socktab.h"

#include <algorithm>

using namespace wc::rt;
namespace tab = wc::tab;

static_assert(WC_RX_DRAIN_SMALL == wc::kRxDrainSmall, "header and kernels agree");
static_assert(sizeof(struct wc_rx_drain_out) == 15 * sizeof(void *), "fifteen pointers");

extern "C" {

// The larger of what the chain's calls ask for (they run one after another on
// the stream and share it); the two launches of the small path use none, but
// ask for the same, so that the function never decreases.
uint64_t wc_rx_drain_scratch(uint64_t n)
{
    return std::max(wc::rxsel_scratch_bytes(n), wc::rxdemux_scratch_bytes(n));
}

int wc_rx_drain(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                const void *d_tab, uint32_t ns, const struct wc_rx_engine *d_eng, uint32_t slot_bytes,
                const struct wc_rx_drain_out *out, void *d_scratch, void *stream)
{
    if (!out || n > kRxListMax || ns > tab::kTabMaxSocks)
        return WC_EINVAL;
    const struct wc_rx_drain_out &o = *out;
    if (!o.start || !o.rcount || !o.nrcount || !o.ucount)
        return WC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const wc::RxDrainArrays a{o.verdict, o.rec,    o.drops,     o.sock,  o.list,
                              o.start,   o.action, o.reply_len, o.rlist, o.rcount,
                              o.nact,    o.nrlist, o.nrcount,   o.ulist, o.ucount};
    if (n != 0) {
        if (slot_bytes > 65535u || !d_base || !d_off || !d_frame_len || !d_tab ||
            ((uintptr_t)d_tab & 3u) || !d_eng || ((uintptr_t)d_eng & 3u))
            return WC_EINVAL;
        if (!o.verdict || !o.rec || ((uintptr_t)o.rec & 15u) || !o.sock || !o.list || !o.action ||
            !o.reply_len || !o.rlist || !o.nact || !o.nrlist || !o.ulist)
            return WC_EINVAL;
        if (!d_scratch || ((uintptr_t)d_scratch & 3u))
            return WC_EINVAL;
    }
    if (n <= WC_RX_DRAIN_SMALL) { // (n = 0: the list launch alone writes the zeros)
        Ready R;
        if (R.rc)
            return R.rc;
        return hip_err(wc::launch_rx_drain(d_base, d_off, d_frame_len, n, d_tab, ns, d_eng,
                                           slot_bytes, a, R.C.nt != 0, st));
    }
    int rc = wc_rx_deliver_ragged(d_base, d_off, d_frame_len, n, o.verdict, o.rec, nullptr, nullptr,
                                  o.drops, nullptr, stream);
    if (rc == WC_OK)
        rc = wc_rx_demux(d_base, d_off, o.rec, n, d_tab, ns, o.sock, o.list, o.start, d_scratch,
                         stream);
    if (rc == WC_OK)
        rc = wc_rx_reply_plan(d_base, d_off, d_frame_len, n, o.verdict, o.sock, d_eng, slot_bytes,
                              o.action, o.reply_len, o.rlist, o.rcount, d_scratch, stream);
    if (rc == WC_OK)
        rc = wc_rx_neigh_plan(d_base, d_off, d_frame_len, n, o.action, d_eng, o.nact, o.nrlist,
                              o.nrcount, o.ulist, o.ucount, d_scratch, stream);
    return rc;
}

} // extern "C"
