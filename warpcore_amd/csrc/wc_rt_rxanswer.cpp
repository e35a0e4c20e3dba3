// wc_rt_rxanswer.cpp -- RX answer (wc_rx_answer_scratch, wc_rx_answer): the
// argument checks -- the chain's own, through the functions its calls use --,
// the two launches of wc_k_rxanswer.hip where each of the three lists has at
// most WC_RX_ANSWER_SMALL entries (and a table at most WC_RX_ANSWER_SMALL_APPLY
// records to apply), and for anything larger the four calls it
// stands for, one after another on the caller's stream (DESIGN.md section
// 4.14).

#include "wc_rt.h"
#include "wc_rx_answer.h"

using namespace wc::rt;
namespace ra = wc::ra;

static_assert(WC_RX_ANSWER_SMALL == ra::kSmall && WC_RX_ANSWER_SMALL_APPLY == ra::kSmallApply,
              "header and kernels agree");

extern "C" {

// What wc_neigh_apply asks for: the two launches of the small path keep the
// entry indices in LDS and use none, but ask for the same, so that the
// function never decreases across the threshold.
uint64_t wc_rx_answer_scratch(uint32_t u_m)
{
    return wc_neigh_apply_scratch(u_m);
}

int wc_rx_answer(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                 const struct wc_rx_engine *d_eng, uint32_t slot_bytes,
                 const struct wc_rx_answer_io *io, void *d_scratch, void *stream)
{
    if (!io || !io->r_built || !io->n_built)
        return WC_EINVAL;
    if (n > kRxListMax || slot_bytes > 65535u)
        return WC_EINVAL;
    const struct wc_rx_answer_io &o = *io;
    // each part's rules are its chain call's
    if (o.r_m != 0 && !o.r_out_len)
        return WC_EINVAL;
    if (o.r_m != 0 && n != 0 &&
        !rx_build_ptrs_ok(d_base, d_off, d_frame_len, o.action, o.rlist, o.rcount, d_eng,
                          o.r_out_base, o.r_out_off))
        return WC_EINVAL;
    if (o.n_m != 0 && !o.n_out_len)
        return WC_EINVAL;
    if (o.n_m != 0 && n != 0 &&
        !rx_build_ptrs_ok(d_base, d_off, d_frame_len, o.nact, o.nrlist, o.nrcount, d_eng,
                          o.n_out_base, o.n_out_off))
        return WC_EINVAL;
    if (o.u_m != 0 &&
        !rx_updates_ptrs_ok(d_base, d_off, d_frame_len, n, o.nact, o.ulist, o.ucount, o.upd))
        return WC_EINVAL;
    const bool apply = o.tab != nullptr && o.u_m != 0;
    if (apply && !neigh_apply_args_ok(o.tab, o.upd, o.ucount, o.u_m, d_scratch))
        return WC_EINVAL;

    const bool small = o.r_m <= WC_RX_ANSWER_SMALL && o.n_m <= WC_RX_ANSWER_SMALL &&
                       o.u_m <= WC_RX_ANSWER_SMALL &&
                       // one workgroup's claim and commit of more records than this measured
                       // slower than wc_neigh_apply's two grids
                       (!apply || o.u_m <= WC_RX_ANSWER_SMALL_APPLY);
    if (!small) {
        int rc = wc_rx_reply_build(d_base, d_off, d_frame_len, n, o.action, o.rlist, o.rcount,
                                   d_eng, o.r_out_base, o.r_out_off, o.r_m, slot_bytes, o.ip_id,
                                   o.r_out_len, o.r_built, stream);
        if (rc == WC_OK)
            rc = wc_rx_neigh_updates(d_base, d_off, d_frame_len, n, o.nact, o.ulist, o.ucount,
                                     o.u_m, o.upd, stream);
        if (rc == WC_OK)
            rc = wc_rx_neigh_build(d_base, d_off, d_frame_len, n, o.nact, o.nrlist, o.nrcount,
                                   d_eng, o.n_out_base, o.n_out_off, o.n_m, slot_bytes,
                                   o.n_out_len, o.n_built, stream);
        if (rc == WC_OK && apply)
            rc = wc_neigh_apply(o.tab, o.upd, o.ucount, o.u_m, o.dropped, d_scratch, stream);
        return rc;
    }

    Ready R;
    if (R.rc)
        return R.rc;
    hipStream_t st = (hipStream_t)stream;
    const wc::RxAnswerArgs a{(const uint8_t *)d_base, d_off, d_frame_len, n,
                             (const uint32_t *)d_eng, slot_bytes,
                             o.action, o.rlist, o.rcount, o.nact, o.nrlist, o.nrcount,
                             o.ulist, o.ucount,
                             (uint8_t *)o.r_out_base, o.r_out_off, o.r_m, o.ip_id, o.r_out_len,
                             o.r_built,
                             (uint8_t *)o.n_out_base, o.n_out_off, o.n_m, o.n_out_len, o.n_built,
                             o.u_m, (uint32_t *)o.upd,
                             (uint32_t *)o.tab, o.dropped};
    // (all three m zero: the apply launch alone writes the two zero counts)
    hipError_t e = wc::launch_rx_answer_frames(a, R.D->cus, st);
    if (e == hipSuccess)
        e = wc::launch_rx_answer_apply(a, st);
    return hip_err(e);
}

} // extern "C"
