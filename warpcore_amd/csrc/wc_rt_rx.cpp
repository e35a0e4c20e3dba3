// wc_rt_rx.cpp -- RX verdict launches (wc_rx_verdict_ragged, wc_rx_deliver_ragged
// and the host paths' RX batches): the default ADAPT mode picks EARLY or HT
// per launch from the tallies earlier launches' tiles stored; and
// wc_rx_select, the index lists over the verdict bytes.

#include "wc_rt.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace wc {
namespace rt __attribute__((visibility("hidden"))) {

std::mutex g_rx_mu;

// One RX verdict launch.  ADAPT (the default): EARLY or HT by the newest
// earlier launch on this device whose tally has arrived (>= 8 sampled tiles,
// or all it will write): EARLY when more than 1 in 8 of its sampled frames
// needed no UDP check (ARP / ICMP / TCP / zero checksums / drops), else HT;
// the previous choice stands until a tally arrives.  The kernel's tally is a
// store per 64 tiles into mapped host memory -- nothing to wait for here,
// and launches stay asynchronous (a tally read while its launch still runs
// is a partial sample).
hipError_t rx_launch(Device &D, const Config &C, const void *base, const uint64_t *offs,
                     const uint16_t *flens, uint64_t n, uint8_t *verdict, uint64_t *drops,
                     hipStream_t st, void *rec)
{
    // A deliver launch (rec): the same choice, among the transposed-header
    // kernels -- WC_RX_HDRT=0 and WC_RX_SKIP=1 are ignored (launch_rx_verdict).
    const int mode = C.rx_mode();
    if (!(mode & wc::kRxAdapt))
        return wc::launch_rx_verdict(base, offs, flens, n, verdict, drops, C.nt != 0, st, mode,
                                     nullptr, 0u, C.rx_grid, rec);
    // (wc_gpu_fini frees the tallies under this lock too: test them inside it)
    std::lock_guard<std::mutex> lk(g_rx_mu);
    if (!D.h_rx_tally[0])
        return wc::launch_rx_verdict(base, offs, flens, n, verdict, drops, C.nt != 0, st,
                                     wc::kRxHdrT, nullptr, 0u, C.rx_grid, rec);
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t from = 0, from_words = 0, from_seen = 0, from_out = 0;
    for (uint32_t back = 1; back < (uint32_t)kRxSets && back <= D.rx_gen; ++back) {
        const uint32_t g = D.rx_gen - back;
        const int set = (int)(g % kRxSets);
        const volatile uint32_t *t = D.h_rx_tally[set];
        uint32_t words = 0, seen = 0, out = 0;
        for (uint32_t i = 0; i < D.rx_words[set]; ++i) {
            const uint32_t w = t[i];
            if ((w >> 16) != (g & 0xFFFFu))
                continue;
            ++words;
            seen += w & 0xFFu;
            out += (w >> 8) & 0xFFu;
        }
        if (words >= 8 || (words && words == D.rx_words[set])) {
            D.rx_early = out * 8u > seen;
            from = g;
            from_words = words;
            from_seen = seen;
            from_out = out;
            break;
        }
    }
    const uint32_t g = ++D.rx_gen;
    const int set = (int)(g % kRxSets);
    const uint64_t tiles = (n + 63) / 64;
    const uint32_t words = (uint32_t)std::min<uint64_t>((tiles + 63) / 64, wc::kRxTallyWords);
    // cleared first: a word older launches left there could carry this
    // launch's 16-bit tag once the tags come round (a late store of launch
    // g - 4 after the clear carries g - 4's tag and is not counted).  The
    // cleared words carry a tag no launch of this set can have -- g's
    // complement, never g's own (a plain 0 is launch g's tag whenever
    // g & 0xFFFF == 0, and its words would count as arrived, empty).
    const uint32_t cleared = ((~g) & 0xFFFFu) << 16;
    for (uint32_t i = 0; i < words; ++i)
        D.h_rx_tally[set][i] = cleared;
    D.rx_words[set] = words;
    if (C.rx_force) // (tools: the tallying kernel with the decision fixed)
        D.rx_early = C.rx_force == 2;
    const int m = wc::kRxHdrT | (D.rx_early ? wc::kRxEarly : 0);
    if (C.rx_trace == 2) { // one summary line per 512 launches
        ++D.rx_nlaunch[D.rx_early ? 1 : 0];
        D.rx_ndecided += from_words != 0;
        if ((g & 511u) == 0) {
            fprintf(stderr, "wccksum rx gen %u: last 512 launches %u HT / %u EARLY, %u decided "
                            "from an arrived tally\n",
                    g, D.rx_nlaunch[0], D.rx_nlaunch[1], D.rx_ndecided);
            D.rx_nlaunch[0] = D.rx_nlaunch[1] = D.rx_ndecided = 0;
        }
    } else if (C.rx_trace)
        fprintf(stderr, "wccksum rx gen %u: %s (tally of gen %u: %u words, %u of %u frames ruled "
                        "out; %.1f us on the host)\n",
                g, D.rx_early ? "EARLY" : "HT", from, from_words, from_out, from_seen,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0)
                    .count());
    return wc::launch_rx_verdict(base, offs, flens, n, verdict, drops, C.nt != 0, st, m,
                                 D.d_rx_tally[set], g & 0xFFFFu, C.rx_grid, rec);
}

} // namespace rt
} // namespace wc

using namespace wc::rt;

extern "C" {

int wc_rx_verdict_ragged(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                         uint64_t n, uint8_t *d_verdict, uint64_t *d_drops, void *stream)
{
    if (n == 0)
        return WC_OK;
    if (!d_base || !d_off || !d_frame_len || !d_verdict)
        return WC_EINVAL;
    Device *D = nullptr;
    Config C;
    int rc = ensure_device(&D, &C);
    if (rc)
        return rc;
    return hip_err(rx_launch(*D, C, d_base, d_off, d_frame_len, n, d_verdict, d_drops,
                             (hipStream_t)stream));
}

uint64_t wc_rx_select_scratch(uint64_t n)
{
    return wc::rxsel_scratch_bytes(n);
}

// Indices are uint32: a batch is at most 2^32 frames.
static constexpr uint64_t kRxSelectMax = 1ull << 32;

// *d_count = 0 for an empty batch (device memory: on the caller's stream).
static int rx_count_zero(uint64_t *d_count, void *stream)
{
    if (!d_count)
        return WC_OK;
    Device *D = nullptr;
    Config C;
    int rc = ensure_device(&D, &C);
    if (rc)
        return rc;
    return hip_err(hipMemsetAsync(d_count, 0, sizeof(uint64_t), (hipStream_t)stream));
}

int wc_rx_select(const uint8_t *d_verdict, uint64_t n, uint32_t mask, uint32_t *d_list,
                 uint64_t *d_count, void *d_scratch, void *stream)
{
    if (n > kRxSelectMax)
        return WC_EINVAL;
    if (n == 0)
        return rx_count_zero(d_count, stream);
    if (!d_verdict || !d_list || !d_count || !d_scratch || ((uintptr_t)d_scratch & 3u))
        return WC_EINVAL;
    Device *D = nullptr;
    Config C;
    int rc = ensure_device(&D, &C);
    if (rc)
        return rc;
    return hip_err(wc::launch_rx_select(d_verdict, n, mask, d_list, d_count, d_scratch,
                                        (hipStream_t)stream));
}

int wc_rx_deliver_ragged(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                         uint64_t n, uint8_t *d_verdict, struct wc_rx_record *d_rec,
                         uint32_t *d_list, uint64_t *d_count, uint64_t *d_drops, void *d_scratch,
                         void *stream)
{
    static_assert(sizeof(struct wc_rx_record) == 16, "one 16-byte store per frame");
    if (n > kRxSelectMax || (d_list != nullptr) != (d_count != nullptr))
        return WC_EINVAL;
    if (n == 0)
        return rx_count_zero(d_count, stream);
    if (!d_base || !d_off || !d_frame_len || !d_verdict || !d_rec || ((uintptr_t)d_rec & 15u))
        return WC_EINVAL;
    if (d_list && (!d_scratch || ((uintptr_t)d_scratch & 3u)))
        return WC_EINVAL;
    Device *D = nullptr;
    Config C;
    int rc = ensure_device(&D, &C);
    if (rc)
        return rc;
    hipError_t e = rx_launch(*D, C, d_base, d_off, d_frame_len, n, d_verdict, d_drops,
                             (hipStream_t)stream, d_rec);
    if (e == hipSuccess && d_list)
        e = wc::launch_rx_select(d_verdict, n, WC_RX_MASK_DELIVER, d_list, d_count, d_scratch,
                                 (hipStream_t)stream);
    return hip_err(e);
}

int wc_rx_deliver_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                       const uint16_t *h_frame_len, uint64_t n, uint8_t *h_verdict,
                       struct wc_rx_record *h_rec, uint32_t *h_list, uint64_t *h_count,
                       uint64_t *h_drops)
{
    if (n > kRxSelectMax || (h_list != nullptr) != (h_count != nullptr))
        return WC_EINVAL;
    if (n == 0) {
        if (h_count)
            *h_count = 0;
        if (h_drops)
            *h_drops = 0;
        return WC_OK;
    }
    if (!h_verdict || !h_rec)
        return WC_EINVAL;
    const int rc = host_batch(h_base, h_bytes, h_off, h_frame_len, n,
                              {{h_verdict, (uint8_t *)h_rec}}, kKindRxDeliver);
    if (rc != WC_OK)
        return rc;
    // The list and the drop count by the calling thread, once the batch has
    // drained: one pass over n bytes (the frames are in host memory anyway).
    uint64_t drops = 0, cnt = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t v = h_verdict[i];
        drops += WC_RX_IS_DROP(v);
        if (h_list && (v == WC_RX_OK || v == WC_RX_OK_NO_CKSUM))
            h_list[cnt++] = (uint32_t)i;
    }
    if (h_count)
        *h_count = cnt;
    if (h_drops)
        *h_drops = drops;
    return WC_OK;
}

} // extern "C"
