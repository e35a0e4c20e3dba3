// wc_rt_rx.cpp -- RX verdict launches (wc_rx_verdict_ragged, wc_rx_deliver_ragged
// and the host paths' RX batches): the default ADAPT mode picks EARLY or HT
// per launch from the tallies earlier launches' tiles stored; and
// wc_rx_select, the index lists over the verdict bytes; and the socket
// demultiplex behind delivery -- the table's host side (wc_rx_socktab_*),
// wc_rx_demux and wc_rx_demux_host.

#include "wc_rt.h"
#include "wc_rx_socktab.h"

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
namespace tab = wc::tab;

extern "C" {

int wc_rx_verdict_ragged(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                         uint64_t n, uint8_t *d_verdict, uint64_t *d_drops, void *stream)
{
    if (n == 0)
        return WC_OK;
    if (!d_base || !d_off || !d_frame_len || !d_verdict)
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(rx_launch(*R.D, R.C, d_base, d_off, d_frame_len, n, d_verdict, d_drops,
                             (hipStream_t)stream));
}

uint64_t wc_rx_select_scratch(uint64_t n)
{
    return wc::rxsel_scratch_bytes(n);
}

// Indices are uint32: a batch is at most 2^32 frames.
static constexpr uint64_t kRxSelectMax = 1ull << 32;

// An empty batch: `bytes` zero bytes at d_out (NULL: nothing to write) --
// device memory, so on the caller's stream.
static int rx_zero_empty(void *d_out, size_t bytes, void *stream)
{
    if (!d_out)
        return WC_OK;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(hipMemsetAsync(d_out, 0, bytes, (hipStream_t)stream));
}

int wc_rx_select(const uint8_t *d_verdict, uint64_t n, uint32_t mask, uint32_t *d_list,
                 uint64_t *d_count, void *d_scratch, void *stream)
{
    if (n > kRxSelectMax)
        return WC_EINVAL;
    if (n == 0)
        return rx_zero_empty(d_count, sizeof(uint64_t), stream);
    if (!d_verdict || !d_list || !d_count || !d_scratch || ((uintptr_t)d_scratch & 3u))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
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
        return rx_zero_empty(d_count, sizeof(uint64_t), stream);
    if (!d_base || !d_off || !d_frame_len || !d_verdict || !d_rec || ((uintptr_t)d_rec & 15u))
        return WC_EINVAL;
    if (d_list && (!d_scratch || ((uintptr_t)d_scratch & 3u)))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e = rx_launch(*R.D, R.C, d_base, d_off, d_frame_len, n, d_verdict, d_drops,
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
    // The drop count and the list by the calling thread, once the batch has
    // drained: a pass each over n bytes (the frames are in host memory anyway).
    if (h_drops)
        *h_drops = rx_count_drops(h_verdict, n);
    if (h_list) {
        uint64_t cnt = 0;
        for (uint64_t i = 0; i < n; ++i)
            if (h_verdict[i] == WC_RX_OK || h_verdict[i] == WC_RX_OK_NO_CKSUM)
                h_list[cnt++] = (uint32_t)i;
        *h_count = cnt;
    }
    return WC_OK;
}

// --- RX socket demultiplex ---------------------------------------------------

uint64_t wc_rx_socktab_bytes(uint32_t ns)
{
    // (past the largest table: still its size, so the function never decreases)
    return 4ull * tab::tab_words(std::min<uint32_t>(ns, tab::kTabMaxSocks));
}

// A socket's canonical key: its own bytes with the ignored ones dropped.
static void sock_key(const struct wc_rx_sock &s, uint32_t k[tab::kTabKeyWords])
{
    uint32_t l[4], r[4];
    memcpy(l, s.laddr, 16);
    memcpy(r, s.raddr, 16);
    tab::tab_key(k, s.af, s.connected, s.lport, s.rport, l, r);
}

int wc_rx_socktab_build(const struct wc_rx_sock *socks, uint32_t ns, void *h_tab)
{
    static_assert(sizeof(struct wc_rx_sock) == 4 * tab::kTabKeyWords, "the key is the struct");
    static_assert(WC_RX_DEMUX_MAX_SOCKS == tab::kTabMaxSocks && WC_RX_SOCK_UNBOUND == tab::kTabUnbound,
                  "header and table agree");
    if (ns > tab::kTabMaxSocks || !h_tab || ((uintptr_t)h_tab & 3u) || (ns && !socks))
        return WC_EINVAL;
    for (uint32_t i = 0; i < ns; ++i)
        if ((socks[i].af != 4 && socks[i].af != 6) || socks[i].connected > 1)
            return WC_EINVAL;
    uint32_t *const t = (uint32_t *)h_tab, *const slot = t + tab::kTabHeaderWords;
    const uint32_t nslots = tab::tab_slots(ns);
    t[0] = tab::kTabMagic, t[1] = nslots, t[2] = ns, t[3] = 0u;
    for (uint32_t q = 0; q < nslots; ++q) {
        uint32_t *const s = slot + q * tab::kTabSlotWords;
        std::fill(s, s + tab::kTabSlotWords, 0u);
        s[tab::kTabKeyWords] = tab::kTabEmpty;
    }
    for (uint32_t i = 0; i < ns; ++i) { // in the caller's order: the same input, the same bytes
        uint32_t k[tab::kTabKeyWords];
        sock_key(socks[i], k);
        uint32_t at = tab::tab_hash(k) & (nslots - 1u);
        while (slot[at * tab::kTabSlotWords + tab::kTabKeyWords] != tab::kTabEmpty) {
            if (!memcmp(slot + at * tab::kTabSlotWords, k, sizeof k))
                return WC_EINVAL; // the same tuple twice
            at = (at + 1u) & (nslots - 1u);
        }
        memcpy(slot + at * tab::kTabSlotWords, k, sizeof k);
        slot[at * tab::kTabSlotWords + tab::kTabKeyWords] = i;
    }
    return WC_OK;
}

// Whether h_tab starts like a blob of wc_rx_socktab_build (for `ns` sockets,
// where the caller names a count).
static bool socktab_ok(const void *h_tab, const uint32_t *ns)
{
    if (!h_tab || ((uintptr_t)h_tab & 3u))
        return false;
    const uint32_t *t = (const uint32_t *)h_tab;
    return t[0] == tab::kTabMagic && t[2] <= tab::kTabMaxSocks && t[1] == tab::tab_slots(t[2]) &&
           (!ns || *ns == t[2]);
}

uint8_t wc_rx_socktab_lookup(const void *h_tab, uint8_t af, const uint8_t *laddr, uint16_t lport,
                             const uint8_t *raddr, uint16_t rport)
{
    if (!socktab_ok(h_tab, nullptr) || (af != 4 && af != 6) || !laddr || !raddr)
        return WC_RX_SOCK_UNBOUND;
    uint32_t l[4] = {}, r[4] = {}, k[tab::kTabKeyWords];
    memcpy(l, laddr, af == 4 ? 4 : 16);
    memcpy(r, raddr, af == 4 ? 4 : 16);
    tab::tab_key(k, af, 1u, lport, rport, l, r);
    const uint32_t *t = (const uint32_t *)h_tab;
    return (uint8_t)tab::tab_lookup(t + tab::kTabHeaderWords, t[1], k);
}

uint64_t wc_rx_demux_scratch(uint64_t n)
{
    return wc::rxdemux_scratch_bytes(n);
}

static constexpr uint64_t kRxStarts = 256; // entries of d_start / h_start

int wc_rx_demux(const void *d_base, const uint64_t *d_off, const struct wc_rx_record *d_rec,
                uint64_t n, const void *d_tab, uint32_t ns, uint8_t *d_sock, uint32_t *d_list,
                uint64_t *d_start, void *d_scratch, void *stream)
{
    if (n > kRxSelectMax || ns > tab::kTabMaxSocks || (d_list != nullptr) != (d_start != nullptr))
        return WC_EINVAL;
    if (n == 0)
        return rx_zero_empty(d_start, kRxStarts * sizeof(uint64_t), stream);
    if (!d_base || !d_off || !d_rec || ((uintptr_t)d_rec & 15u) || !d_tab ||
        ((uintptr_t)d_tab & 3u) || !d_sock)
        return WC_EINVAL;
    if (d_list && (!d_scratch || ((uintptr_t)d_scratch & 3u)))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(wc::launch_rx_demux(d_base, d_off, d_rec, n, d_tab, ns, d_sock, d_list, d_start,
                                       d_scratch, (hipStream_t)stream));
}

int wc_rx_demux_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                     const uint16_t *h_frame_len, uint64_t n, const void *h_tab, uint32_t ns,
                     uint8_t *h_verdict, struct wc_rx_record *h_rec, uint8_t *h_sock,
                     uint32_t *h_list, uint64_t *h_start, uint64_t *h_drops)
{
    if (n > kRxSelectMax || ns > tab::kTabMaxSocks || (h_list != nullptr) != (h_start != nullptr))
        return WC_EINVAL;
    if (n == 0) {
        if (h_start)
            std::fill(h_start, h_start + kRxStarts, 0ull);
        if (h_drops)
            *h_drops = 0;
        return WC_OK;
    }
    if (!h_verdict || !h_rec || !h_sock || !socktab_ok(h_tab, &ns))
        return WC_EINVAL;
    const int rc = host_batch(h_base, h_bytes, h_off, h_frame_len, n,
                              {{h_verdict, (uint8_t *)h_rec, h_sock}}, kKindRxDemux, h_tab, ns);
    if (rc != WC_OK)
        return rc;
    if (h_drops)
        *h_drops = rx_count_drops(h_verdict, n);
    if (!h_list)
        return WC_OK;
    // The per-socket runs by the calling thread: one counting pass over the n
    // socket bytes, the starts, then every delivered index to its run's next
    // place -- ascending i, so each run is in ring order.
    uint64_t cnt[kRxStarts] = {}, next[kRxStarts];
    for (uint64_t i = 0; i < n; ++i)
        ++cnt[h_sock[i]];
    cnt[WC_RX_SOCK_NONE] = 0; // (not delivered: in no run)
    uint64_t at = 0;
    for (uint64_t s = 0; s < ns; ++s) {
        h_start[s] = next[s] = at;
        at += cnt[s];
    }
    for (uint64_t s = ns; s < kRxStarts - 1; ++s)
        h_start[s] = at;
    next[WC_RX_SOCK_UNBOUND] = at;
    h_start[kRxStarts - 1] = at + cnt[WC_RX_SOCK_UNBOUND];
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t s = h_sock[i];
        if (s < ns || s == WC_RX_SOCK_UNBOUND)
            h_list[next[s]++] = (uint32_t)i;
    }
    return WC_OK;
}

} // extern "C"
