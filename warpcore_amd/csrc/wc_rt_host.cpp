// wc_rt_host.cpp -- host-memory batches (wc_cksum_host, wc_cksum_ip_udp_host,
// wc_rx_verdict_host, wc_rx_deliver_host, wc_rx_demux_host, the seal's compute pass,
// wc_host_register): the
// resident server or one zero-copy launch for a small registered batch, else
// the in-place stream or the pipelined path (hipMemcpyAsync H2D, kernel, D2H)
// through pinned staging.  All three launch paths keep their per-batch arrays
// in a BufSet (one alloc, free and copy_out), the chunked two in a Slot (one
// drain), and pick a kind's result arrays from out_row (wc_rt.h).

#include "wc_rt.h"
#include "wc_rx_socktab.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

namespace wc {
namespace rt __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------------------
// The per-batch arrays (BufSet) and the launch in flight on them (Slot).

// One array of a set, in the set's flavour, on the current device.
template <class T>
static bool buf_alloc(bool mapped, T *&h, T *&d, uint64_t bytes)
{
    const unsigned fl = mapped ? hipHostMallocMapped | hipHostMallocCoherent : 0;
    if (hipHostMalloc((void **)&h, bytes, fl) != hipSuccess)
        return false;
    return (mapped ? hipHostGetDevicePointer((void **)&d, h, 0)
                   : hipMalloc((void **)&d, bytes)) == hipSuccess;
}

int BufSet::alloc(uint64_t pkts, bool mapped_pinned)
{
    mapped = mapped_pinned;
    this->pkts = pkts;
    bool ok = buf_alloc(mapped, h.off, d.off, pkts * 8);
    ok = ok && buf_alloc(mapped, h.len, d.len, pkts * 2);
    for (int k = 0; k < kOuts && ok; ++k)
        ok = buf_alloc(mapped, h.out[k], d.out[k], pkts * kOutCap.w[k]);
    if (!ok)
        free();
    return ok ? WC_OK : WC_ENOMEM;
}

int BufSet::need(int kind)
{
    if (!kind_has_rec(kind) || h.rec)
        return WC_OK;
    if (buf_alloc(mapped, h.rec, d.rec, pkts * out_row(kKindRxDeliver).w[1]))
        return WC_OK;
    if (!mapped)
        (void)hipFree(d.rec);
    (void)hipHostFree(h.rec);
    h.rec = d.rec = nullptr;
    return WC_ENOMEM;
}

void BufSet::free()
{
    if (!mapped) { // (a mapped set's device view is the host memory's own)
        (void)hipFree(d.off);
        (void)hipFree(d.len);
        for (uint8_t *p : d.out)
            (void)hipFree(p);
        (void)hipFree(d.rec);
    }
    (void)hipHostFree(h.off);
    (void)hipHostFree(h.len);
    for (uint8_t *p : h.out)
        (void)hipHostFree(p);
    (void)hipHostFree(h.rec);
    *this = BufSet{};
}

void BufSet::copy_out(int kind, const HostOuts &outs, uint64_t lo, uint64_t n) const
{
    const OutRow row = out_row(kind);
    for (int k = 0; k < kOuts; ++k)
        if (row.w[k])
            memcpy(outs.p[k] + lo * row.w[k], (const void *)h.out_of(kind, k), n * row.w[k]);
}

int Slot::init(uint64_t pkts, bool mapped_pinned)
{
    if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess)
        return WC_ENOMEM;
    return b.alloc(pkts, mapped_pinned);
}

void Slot::free()
{
    if (done)
        (void)hipEventDestroy(done);
    b.free();
    *this = Slot{};
}

int Slot::drain(int kind, const HostOuts &outs)
{
    if (!pend)
        return WC_OK;
    const int rc = hip_err(hipEventSynchronize(done));
    if (rc)
        return rc;
    b.copy_out(kind, outs, lo, n);
    pend = false;
    return WC_OK;
}

// ---------------------------------------------------------------------------
// Host-memory pipeline.

// Frees whatever a (possibly partly built) pipeline holds.
void pipe_free(HostPipe &P)
{
    for (PipeSlot &s : P.slot) {
        if (s.st)
            (void)hipStreamSynchronize(s.st);
        (void)hipFree(s.d_bytes);
        (void)hipHostFree(s.h_bytes);
        s.free();
        if (s.st)
            (void)hipStreamDestroy(s.st);
    }
    P = HostPipe{};
}

// Streams, events and staging of one host pipeline, created on the current
// device.
int pipe_init_locked(HostPipe &P)
{
    if (P.ready)
        return WC_OK;
    for (PipeSlot &s : P.slot) {
        if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess ||
            hipMalloc((void **)&s.d_bytes, kChunkBytes + 64) != hipSuccess ||
            hipHostMalloc((void **)&s.h_bytes, kChunkBytes + 64, 0) != hipSuccess ||
            s.init(kChunkPkts, false) != WC_OK) {
            pipe_free(P);
            return WC_ENOMEM;
        }
    }
    P.ready = true;
    return WC_OK;
}

void zc_free(ZeroCopy &Z)
{
    if (Z.st) {
        (void)hipStreamSynchronize(Z.st);
        (void)hipStreamDestroy(Z.st);
    }
    Z.b.free();
    Z = ZeroCopy{};
}

int zc_init_locked(Device &D)
{
    ZeroCopy &Z = D.zc;
    if (Z.ready)
        return WC_OK;
    if (hipStreamCreateWithFlags(&Z.st, hipStreamNonBlocking) != hipSuccess ||
        Z.b.alloc(kZcPkts, true) != WC_OK) {
        zc_free(Z);
        return WC_ENOMEM;
    }
    Z.ready = true;
    return WC_OK;
}

// Address on the CURRENT device of host range [p, p + bytes) if it lies
// inside one registered region, else nullptr.  The region was registered
// portable and mapped; its device address is looked up for this device the
// first time (a batch may run on a shard device other than the one current
// at wc_host_register).
const uint8_t *registered_dptr_locked(const void *p, uint64_t bytes)
{
    const uintptr_t a = (uintptr_t)p;
    auto it = g_registered.upper_bound(a);
    if (it == g_registered.begin())
        return nullptr;
    --it;
    if (a < it->first || a + bytes > it->first + it->second.bytes)
        return nullptr;
    int dev = 0;
    if (current_device(&dev) != WC_OK)
        return nullptr;
    const uint8_t *&d = it->second.dptr[dev];
    if (!d) {
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, (void *)it->first, 0) != hipSuccess)
            return nullptr;
        d = (const uint8_t *)dp;
    }
    return d + (a - it->first);
}

// Bytes the reference reads for one packet (payload_cksum reads the IPv4
// header fields up to byte 19 whatever len is, in_cksum.c:149-151).
uint64_t span_of(uint16_t len, int kind)
{
    return kind == WC_CKSUM_PAYLOAD || kind == kKindFused ? std::max<uint64_t>(len, 20) : len;
}

// Bytes the fused TX pair reads of the packet at p (whose first
// span_of(len, kKindFused) bytes are known to be readable): payload_cksum's,
// and the IPv4 header's hl bytes ip_cksum sums (ip4.c:184-186) when they run
// past them (options behind a short len).
uint64_t fused_span(const uint8_t *p, uint16_t len)
{
    const uint64_t s = span_of(len, kKindFused);
    if (s >= 60) // (no IPv4 header is longer: the packet's byte need not be read)
        return s;
    return (p[0] >> 4) == 4 ? std::max<uint64_t>(s, (uint64_t)(p[0] & 15u) * 4u) : s;
}

// One device launch over a ragged batch of `kind` (a checksum kind, RX
// verdicts -- lengths are frame lengths --, the fused pair or the seal's
// compute pass): offsets, lengths and result arrays are b's device view.
int run_ragged_any(Device &D, const Config &C, const uint8_t *d_base, const BufView &b,
                   uint64_t n, int kind, bool zero_copy, hipStream_t st)
{
    uint16_t *const d_out = (uint16_t *)b.out[0], *const d_out_hdr = (uint16_t *)b.out[1];
    if (kind == kKindRx)
        return hip_err(rx_launch(D, C, d_base, b.off, b.len, n, b.out[0], nullptr, st));
    if (kind == kKindRxDeliver)
        return hip_err(rx_launch(D, C, d_base, b.off, b.len, n, b.out[0], nullptr, st, b.rec));
    if (kind == kKindRxDemux) { // the key kernel behind the DELIVER kernel: ids, no list
        hipError_t e = rx_launch(D, C, d_base, b.off, b.len, n, b.out[0], nullptr, st, b.rec);
        if (e == hipSuccess)
            e = wc::launch_rx_demux(d_base, b.off, b.rec, n, D.d_socktab, D.socktab_ns, b.out[2],
                                    nullptr, nullptr, nullptr, st);
        return hip_err(e);
    }
    if (kind_is_tx(kind)) // compute only: the calling thread makes the stores (wc_rt_tx.cpp)
        return hip_err(wc::launch_tx_seal(
            const_cast<uint8_t *>(d_base), b.off, b.len, n,
            wc::kTxNoStore | (kind == kKindTxZero ? wc::kTxZeroUdp : 0u), b.out[2], d_out_hdr,
            d_out, nullptr, C.nt != 0, st));
    const bool fused = kind == kKindFused;
    const int k = fused ? WC_CKSUM_PAYLOAD : kind;
    const Plan p = plan_ragged(D, C, n, k, zero_copy, fused);
    wc::LaunchArgs a{d_base, 0,       0, b.off, b.len, n,         d_out,
                     nullptr, k,       true,  false, C.nt != 0, C.flat_tpw,
                     fused ? d_out_hdr : nullptr};
    return run(D, C, a, p, st);
}

// Small registered batch: one launch reading host memory in place.
int host_zero_copy(Device &D, const uint8_t *dbase, const uint64_t *h_off,
                   const uint16_t *h_len, uint64_t n, const HostOuts &outs, int kind)
{
    int rc = zc_init_locked(D);
    if (rc)
        return rc;
    ZeroCopy &Z = D.zc;
    rc = Z.b.need(kind);
    if (rc)
        return rc;
    memcpy(Z.b.h.off, h_off, n * 8);
    memcpy(Z.b.h.len, h_len, n * 2);
    rc = run_ragged_any(D, g_cfg, dbase, Z.b.d, n, kind, true, Z.st);
    if (rc == WC_OK)
        rc = hip_err(hipStreamSynchronize(Z.st));
    if (rc == WC_OK)
        Z.b.copy_out(kind, outs, 0, n);
    return rc;
}

void zs_free(ZcStream &S)
{
    if (S.st)
        (void)hipStreamSynchronize(S.st);
    for (Slot &s : S.slot)
        s.free();
    if (S.st)
        (void)hipStreamDestroy(S.st);
    S = ZcStream{};
}

int zs_init_locked(Device &D)
{
    ZcStream &S = D.zs;
    if (S.ready)
        return WC_OK;
    if (hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking) != hipSuccess ||
        S.slot[0].init(kZsPkts, true) != WC_OK || S.slot[1].init(kZsPkts, true) != WC_OK) {
        zs_free(S);
        return WC_ENOMEM;
    }
    S.ready = true;
    return WC_OK;
}

// A large batch in a registered region (ZcStream): chunk k's launch reads
// its packets in place while the host writes chunk k + 1's offsets and
// lengths into the other buffer and copies chunk k - 1's results out.
int host_zc_stream(Device &D, const uint8_t *dbase, const uint64_t *h_off,
                   const uint16_t *h_len, uint64_t n, const HostOuts &outs, int kind)
{
    int rc = zs_init_locked(D);
    if (rc)
        return rc;
    ZcStream &S = D.zs;
    int b = 0;
    const uint64_t per = g_cfg.zs_pkts;
    for (uint64_t i = 0; i < n && rc == WC_OK; i += per, b ^= 1) {
        Slot &s = S.slot[b];
        const uint64_t cnt = std::min(per, n - i);
        rc = s.drain(kind, outs); // (chunk k - 2's results: its buffers are free again)
        if (rc == WC_OK)
            rc = s.b.need(kind);
        if (rc)
            break;
        memcpy(s.b.h.off, h_off + i, cnt * 8);
        memcpy(s.b.h.len, h_len + i, cnt * 2);
        rc = run_ragged_any(D, g_cfg, dbase, s.b.d, cnt, kind, true, S.st);
        if (rc == WC_OK)
            rc = hip_err(hipEventRecord(s.done, S.st));
        if (rc == WC_OK)
            s.mark(i, cnt);
    }
    if (rc == WC_OK)
        rc = S.slot[b].drain(kind, outs); // the older of the two in flight first
    if (rc == WC_OK)
        rc = S.slot[b ^ 1].drain(kind, outs);
    if (rc != WC_OK) { // (nothing may still write the mapped buffers the next call refills)
        (void)hipStreamSynchronize(S.st);
        S.slot[0].pend = S.slot[1].pend = false;
    }
    return rc;
}

// Library-owned staging workers.  Pageable input reaches the GPU through
// the pinned staging ring, and copying it there was the end-to-end path's
// limit on one thread (24.6-28.9 GB/s against ~55 GB/s for DMA from
// registered memory) -- for every shard of
// wc_cksum_host_multi alike, since the engine thread stages them all.  The
// copy of each chunk is split over W workers plus the calling thread
// (WC_STAGE_THREADS, default min(8, cores - 1); 0 = the calling thread
// alone).  Created at the first pageable chunk, joined at exit.
class StagePool {
public:
    explicit StagePool(int workers)
    {
        for (int i = 0; i < workers; ++i)
            th_.emplace_back([this] { loop(); });
    }
    ~StagePool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_)
            t.join();
    }
    int width() const { return (int)th_.size() + 1; }
    // fn(0) .. fn(parts - 1), the calling thread taking its share; returns
    // when all are done.
    void run(int parts, const std::function<void(int)> &fn)
    {
        if (parts <= 1 || th_.empty()) {
            for (int i = 0; i < parts; ++i)
                fn(i);
            return;
        }
        std::unique_lock<std::mutex> lk(mu_);
        job_ = &fn;
        parts_ = parts;
        next_ = 0;
        pending_ = parts;
        ++gen_;
        cv_.notify_all();
        while (next_ < parts_) {
            const int i = next_++;
            lk.unlock();
            fn(i);
            lk.lock();
            --pending_;
        }
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }

private:
    void loop()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || (gen_ != seen && job_ && next_ < parts_); });
            if (stop_)
                return;
            seen = gen_;
            while (job_ && next_ < parts_) {
                const int i = next_++;
                const std::function<void(int)> *fn = job_;
                lk.unlock();
                (*fn)(i);
                lk.lock();
                if (--pending_ == 0)
                    done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int parts_ = 0, next_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

StagePool &stage_pool()
{
    static StagePool pool([] {
        const char *v = getenv("WC_STAGE_THREADS");
        if (v && *v)
            return std::max(0, atoi(v));
        const int hw = (int)std::thread::hardware_concurrency();
        return std::max(0, std::min(8, hw - 1));
    }());
    return pool;
}

// memcpy of `bytes` split over the staging pool (pieces of >= 2 MiB).
void stage_copy(void *dst, const void *src, uint64_t bytes)
{
    StagePool &P = stage_pool();
    constexpr uint64_t kPiece = 2ull << 20;
    const int parts = (int)std::min<uint64_t>((uint64_t)P.width(), (bytes + kPiece - 1) / kPiece);
    if (parts <= 1) {
        memcpy(dst, src, bytes);
        return;
    }
    const uint64_t step = ((bytes + parts - 1) / parts + 63) & ~63ull;
    P.run(parts, [&](int i) {
        const uint64_t lo = std::min(bytes, (uint64_t)i * step);
        const uint64_t hi = std::min(bytes, lo + step);
        memcpy((uint8_t *)dst + lo, (const uint8_t *)src + lo, hi - lo);
    });
}

// Pipelined path: chunks of packets go through kPipe streams, each chunk
// H2D -> kernel -> D2H.  An ascending batch ships the byte range its chunk
// covers (straight from registered memory, else via pinned staging); any
// other order is gathered packet by packet into pinned staging first.
//
// A PipeRun walks packets [i, hi) of a batch through one HostPipe on one
// device, one chunk per step(), so a single host thread can interleave the
// runs of several devices (wc_cksum_host_multi): while it stages device g's
// next chunk, the other devices' copies and kernels are in flight.
// Bytes packet j's check reads (the fused pair: also its IPv4 header).
uint64_t PipeRun::span(uint64_t j) const
{
    return kind == kKindFused ? fused_span(hb + h_off[j], h_len[j]) : span_of(h_len[j], kind);
}

// On any error, wait for every slot's in-flight copies and kernel before
// returning: they use the library's pinned staging, which the next call
// rewrites with plain memcpy.
int PipeRun::fail(int rc)
{
    for (PipeSlot &s : P->slot) {
        (void)hipStreamSynchronize(s.st);
        s.pend = false;
    }
    return rc;
}

// Stage and enqueue the next chunk (caller: current device = dev).
int PipeRun::step()
{
    PipeSlot &S = P->slot[slot];
    int rc = S.drain(kind, outs);
    if (rc == WC_OK)
        rc = S.b.need(kind);
    if (rc)
        return rc;
    const BufView &sh = S.b.h, &sd = S.b.d;
    const uint64_t i0 = i;
    uint64_t j = i, bytes = 0;
    const uint8_t *src = nullptr;
    if (ascending) {
        const uint64_t lo = h_off[i];
        uint64_t top = lo;
        while (j < hi && j - i0 < kChunkPkts) {
            const uint64_t e = h_off[j] + span(j);
            if (std::max(top, e) - lo > kChunkBytes && j > i0)
                break;
            top = std::max(top, e);
            sh.off[j - i0] = h_off[j] - lo;
            sh.len[j - i0] = h_len[j];
            ++j;
        }
        bytes = top - lo;
        src = hb + lo;
        if (!registered) {
            stage_copy(S.h_bytes, src, bytes);
            src = S.h_bytes;
        }
    } else {
        // Rebased offsets first (a prefix sum), then the packet copies
        // in parallel ranges of the staging pool.
        while (j < hi && j - i0 < kChunkPkts) {
            const uint64_t sp = span(j);
            if (bytes + sp > kChunkBytes && j > i0)
                break;
            sh.off[j - i0] = bytes;
            sh.len[j - i0] = h_len[j];
            bytes += sp;
            ++j;
        }
        const uint64_t cnt = j - i0;
        StagePool &pool = stage_pool();
        const int parts = (int)std::min<uint64_t>((uint64_t)pool.width(), (cnt + 4095) / 4096);
        uint8_t *dst = S.h_bytes;
        const uint64_t *roff = sh.off;
        auto gather = [&](int t) {
            const uint64_t a = cnt * (uint64_t)t / (uint64_t)parts;
            const uint64_t b = cnt * (uint64_t)(t + 1) / (uint64_t)parts;
            for (uint64_t q = a; q < b; ++q)
                memcpy(dst + roff[q], hb + h_off[i0 + q], span(i0 + q));
        };
        pool.run(std::max(parts, 1), gather);
        src = S.h_bytes;
    }
    const uint64_t cnt = j - i0;
    hipStream_t st = S.st;
    hipError_t e = hipMemcpyAsync(S.d_bytes, src, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sd.off, sh.off, cnt * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sd.len, sh.len, cnt * 2, hipMemcpyHostToDevice, st);
    if (e != hipSuccess)
        return hip_err(e);
    rc = run_ragged_any(*D, g_cfg, S.d_bytes, sd, cnt, kind, false, st);
    if (rc)
        return rc;
    const OutRow row = out_row(kind);
    for (int k = 0; k < kOuts && e == hipSuccess; ++k)
        if (row.w[k])
            e = hipMemcpyAsync(sh.out_of(kind, k), sd.out_of(kind, k), cnt * row.w[k],
                               hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipEventRecord(S.done, st);
    if (e != hipSuccess)
        return hip_err(e);
    S.mark(i0, cnt);
    i = j;
    slot = (slot + 1) % kPipe;
    return WC_OK;
}

int PipeRun::finish()
{
    for (int s = 0; s < kPipe; ++s) {
        int rc = P->slot[(slot + s) % kPipe].drain(kind, outs);
        if (rc)
            return rc;
    }
    return WC_OK;
}

// Every packet of a host batch inside [0, h_bytes); its order and bytes.
bool host_batch_ok(const uint8_t *hb, uint64_t h_bytes, const uint64_t *h_off,
                   const uint16_t *h_len, uint64_t n, int kind, bool *ascending, uint64_t *total,
                   uint64_t *range)
{
    bool asc = true;
    uint64_t tot = 0, lo = ~0ull, hi = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t o = h_off[i];
        uint64_t sp = span_of(h_len[i], kind);
        if (o > h_bytes || sp > h_bytes - o)
            return false;
        if (kind == kKindFused) { // (its first sp >= 20 bytes are in range)
            sp = fused_span(hb + o, h_len[i]);
            if (sp > h_bytes - o)
                return false;
        }
        asc &= i == 0 || o >= h_off[i - 1];
        tot += sp;
        lo = std::min(lo, o);
        hi = std::max(hi, o + sp);
    }
    *ascending = asc;
    *total = tot;
    if (range)
        *range = n ? hi - lo : 0;
    return true;
}

void shard_range(uint64_t n, int g, int G, uint64_t *lo, uint64_t *hi)
{
    // n * g / G without overflow for any uint64 n
    *lo = (uint64_t)((unsigned __int128)n * (unsigned)g / (unsigned)G);
    *hi = (uint64_t)((unsigned __int128)n * (unsigned)(g + 1) / (unsigned)G);
}

int host_pipeline(Device &D, const HostBatch &b, uint64_t n)
{
    PipeRun r{b, &D, &D.pipe, 0, 0, n};
    while (!r.done()) {
        const int rc = r.step();
        if (rc)
            return r.fail(rc);
    }
    const int rc = r.finish();
    return rc ? r.fail(rc) : WC_OK;
}

// wc_cksum_host / wc_rx_verdict_host / wc_cksum_ip_udp_host / the seal's
// compute pass: a host-memory batch on the current device -- the resident
// server or one zero-copy launch for a small registered batch, else the
// in-place stream or the pipeline.
int host_batch(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
               const uint16_t *h_len, uint64_t n, const HostOuts &outs, int kind,
               const void *h_tab, uint32_t ns)
{
    if (n == 0)
        return WC_OK;
    if (!h_base || !h_off || !h_len)
        return WC_EINVAL;
    for (int k = 0; k < kOuts; ++k)
        if (out_row(kind).w[k] && !outs.p[k])
            return WC_EINVAL;
    bool ascending = true;
    uint64_t total = 0, range = 0;
    if (!host_batch_ok((const uint8_t *)h_base, h_bytes, h_off, h_len, n, kind, &ascending,
                       &total, &range))
        return WC_EINVAL;
    // Packets covering less than 7/8 of their byte range (netmap slots: 1472
    // of 2048 B) are sparse: the pipeline would ship the gaps too.
    const bool sparse = total < range - range / 8;

    std::lock_guard<FairMutex> lk(g_mu);
    Device *D = nullptr;
    int rc = init_locked(-1, &D);
    if (rc)
        return rc;
    if (kind == kKindRxDemux) {
        // The table, once per call: no launch of an earlier call is in flight
        // (host calls are synchronous and hold g_mu).
        const uint64_t cap = 4ull * wc::tab::tab_words(wc::tab::kTabMaxSocks);
        if (!D->d_socktab && hipMalloc(&D->d_socktab, cap) != hipSuccess) {
            D->d_socktab = nullptr;
            return WC_ENOMEM;
        }
        rc = hip_err(hipMemcpy(D->d_socktab, h_tab, 4ull * wc::tab::tab_words(ns),
                               hipMemcpyHostToDevice));
        if (rc)
            return rc;
        D->socktab_ns = ns;
    }
    const uint8_t *dbase = registered_dptr_locked(h_base, h_bytes);
    if (dbase && !kind_is_tx(kind) && !kind_has_rec(kind) && g_cfg.serve &&
        server_enabled_locked() &&
        n <= (uint64_t)g_cfg.serve_max) {
        bool fits = true; // (a fused header adds at most 40 bytes to the span)
        for (uint64_t i = 0; i < n && fits; ++i)
            fits = span_of(h_len[i], kind) + (kind == kKindFused ? 40u : 0u) <= wc::kSrvMaxBytes;
        int dev = 0;
        if (fits && current_device(&dev) == WC_OK) {
            rc = serve_batch(*D, dev, dbase, h_off, h_len, n, outs, kind);
            if (rc != kSrvFallback)
                return rc;
        }
    }
    if (dbase && n <= kZcPkts && total <= (uint64_t)g_cfg.zc_bytes)
        return host_zero_copy(*D, dbase, h_off, h_len, n, outs, kind);
    // A large registered batch: sparse or in any order, the kernels read its
    // packets in place (only the lines they touch cross the link); dense and
    // ascending, the pipeline's range DMA is a little faster (C2 bytes from a
    // registered region: 54.5 vs 52.9 GB/s, the three sparse ring calls 39 ->
    // 46-47 GB/s: profiles/e2e_r06b.log).
    if (dbase && g_cfg.zc_stream && (sparse || !ascending))
        return host_zc_stream(*D, dbase, h_off, h_len, n, outs, kind);
    rc = pipe_init_locked(D->pipe);
    if (rc)
        return rc;
    // (pageable and sparse: gathered packet by packet into the staging, not
    // the whole range with its gaps)
    return host_pipeline(*D, {(const uint8_t *)h_base, dbase != nullptr, ascending && !sparse,
                              h_off, h_len, kind, outs}, n);
}

} // namespace rt
} // namespace wc

using namespace wc::rt;

extern "C" {

int wc_host_register(void *h_ptr, uint64_t bytes)
{
    if (!h_ptr || !bytes)
        return WC_EINVAL;
    std::lock_guard<FairMutex> lk(g_mu);
    Device *D = nullptr;
    int rc = init_locked(-1, &D);
    if (rc)
        return rc;
    // The resident server grid would hold up a device-wide synchronisation
    // that (un)registering may do until the idle watcher stopped it -- and
    // the watcher waits for g_mu, held here.  Stop it first; the next small
    // call starts it again.
    server_stop_all_locked();
    // Registering a base address again always pins the pages mapped there
    // NOW: the caller may have freed the old region without
    // wc_host_unregister and got a new buffer at the same address, whose
    // pages the old registration (and its cached device addresses) do not
    // cover.  So the old registration is dropped and the range registered
    // afresh; if that fails, the old range is registered again so a live
    // region keeps working, and the error is returned.
    uint64_t old_bytes = 0;
    auto it = g_registered.find((uintptr_t)h_ptr);
    if (it != g_registered.end()) {
        old_bytes = it->second.bytes;
        g_registered.erase(it);
        (void)hipHostUnregister(h_ptr);
    }
    const unsigned flags = hipHostRegisterMapped | hipHostRegisterPortable;
    auto pin = [&](uint64_t nb) -> hipError_t {
        // Portable: every device (wc_cksum_host_multi's shards) may DMA from it.
        hipError_t e = hipHostRegister(h_ptr, nb, flags);
        if (e != hipSuccess)
            return e;
        void *dptr = nullptr;
        e = hipHostGetDevicePointer(&dptr, h_ptr, 0);
        if (e != hipSuccess) {
            (void)hipHostUnregister(h_ptr);
            return e;
        }
        Registration reg;
        reg.bytes = nb;
        int dev = 0;
        if (current_device(&dev) == WC_OK)
            reg.dptr[dev] = (const uint8_t *)dptr;
        g_registered[(uintptr_t)h_ptr] = reg;
        return hipSuccess;
    };
    const hipError_t e = pin(bytes);
    if (e != hipSuccess && old_bytes)
        (void)pin(old_bytes);
    return hip_err(e);
}

int wc_host_unregister(void *h_ptr)
{
    if (!h_ptr)
        return WC_EINVAL;
    std::lock_guard<FairMutex> lk(g_mu);
    auto it = g_registered.find((uintptr_t)h_ptr);
    if (it == g_registered.end())
        return WC_EINVAL;
    g_registered.erase(it);
    server_stop_all_locked(); // (see wc_host_register)
    return hip_err(hipHostUnregister(h_ptr));
}

int wc_cksum_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                  const uint16_t *h_len, uint64_t n, uint16_t *h_out, int kind)
{
    if (kind != WC_CKSUM_IP && kind != WC_CKSUM_PAYLOAD)
        return WC_EINVAL;
    return host_batch(h_base, h_bytes, h_off, h_len, n, {{(uint8_t *)h_out}}, kind);
}

int wc_cksum_ip_udp_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                         const uint16_t *h_len, uint64_t n, uint16_t *h_out_ip_hdr,
                         uint16_t *h_out_payload)
{
    if (n && (!h_out_ip_hdr || !h_out_payload))
        return WC_EINVAL;
    return host_batch(h_base, h_bytes, h_off, h_len, n,
                      {{(uint8_t *)h_out_payload, (uint8_t *)h_out_ip_hdr}}, kKindFused);
}

int wc_rx_verdict_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                       const uint16_t *h_frame_len, uint64_t n, uint8_t *h_verdict,
                       uint64_t *h_drops)
{
    if (n && !h_verdict)
        return WC_EINVAL;
    const int rc = host_batch(h_base, h_bytes, h_off, h_frame_len, n, {{h_verdict}}, kKindRx);
    if (rc == WC_OK && h_drops)
        *h_drops = rx_count_drops(h_verdict, n);
    return rc;
}

} // extern "C"
