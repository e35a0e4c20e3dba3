// wc_cksum_kernels.h -- internal interface between the C-ABI layer
// (wc_cksum_api.cpp) and the gfx950 kernels (wc_k_*.hip, wc_device.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define WC_KIND_IP 0
#define WC_KIND_PAYLOAD 1

// Every (group width, chunk loads per lane, packets per group-iteration)
// shape the strided planner may pick (wc_cksum_api.cpp: shape_for_chunks) or
// WC_SHAPE may request; each is instantiated for ip_cksum (masked and
// aligned-unmasked) and payload_cksum, with temporal and nontemporal loads.
#define WC_SHAPE_LIST                                                          \
    WC_SHAPE(4, 1, 1)                                                          \
    WC_SHAPE(4, 1, 2)                                                          \
    WC_SHAPE(4, 1, 4)                                                          \
    WC_SHAPE(4, 1, 8)                                                          \
    WC_SHAPE(4, 2, 2)                                                          \
    WC_SHAPE(4, 2, 4)                                                          \
    WC_SHAPE(8, 1, 2)                                                          \
    WC_SHAPE(8, 2, 4)                                                          \
    WC_SHAPE(8, 3, 2)                                                          \
    WC_SHAPE(8, 3, 4)                                                          \
    WC_SHAPE(4, 5, 4)                                                          \
    WC_SHAPE(8, 5, 2)                                                          \
    WC_SHAPE(8, 6, 2)                                                          \
    WC_SHAPE(8, 6, 1)                                                          \
    WC_SHAPE(16, 3, 2)                                                         \
    WC_SHAPE(16, 1, 2)                                                         \
    WC_SHAPE(16, 2, 2)                                                         \
    WC_SHAPE(16, 3, 1)                                                         \
    WC_SHAPE(32, 1, 2)                                                         \
    WC_SHAPE(32, 1, 4)                                                         \
    WC_SHAPE(32, 2, 1)                                                         \
    WC_SHAPE(4, 1, 16)                                                         \
    WC_SHAPE(8, 1, 4)                                                          \
    WC_SHAPE(8, 1, 8)                                                          \
    WC_SHAPE(16, 1, 4)                                                         \
    WC_SHAPE(16, 1, 8)                                                         \
    WC_SHAPE(16, 2, 4)                                                         \
    WC_SHAPE(16, 3, 4)                                                         \
    WC_SHAPE(16, 4, 2)                                                         \
    WC_SHAPE(16, 4, 4)                                                         \
    WC_SHAPE(16, 5, 2)                                                         \
    WC_SHAPE(16, 5, 4)                                                         \
    WC_SHAPE(16, 6, 2)                                                         \
    WC_SHAPE(16, 6, 4)                                                         \
    WC_SHAPE(32, 2, 2)                                                         \
    WC_SHAPE(32, 2, 4)                                                         \
    WC_SHAPE(32, 3, 1)                                                         \
    WC_SHAPE(32, 3, 2)                                                         \
    WC_SHAPE(32, 3, 4)                                                         \
    WC_SHAPE(32, 3, 8)                                                         \
    WC_SHAPE(32, 4, 1)                                                         \
    WC_SHAPE(32, 4, 2)                                                         \
    WC_SHAPE(64, 2, 1)                                                         \
    WC_SHAPE(64, 2, 2)                                                         \
    WC_SHAPE(32, 18, 1)                                                        \
    WC_SHAPE(64, 4, 1)                                                         \
    WC_SHAPE(64, 9, 1)                                                         \
    WC_SHAPE(64, 9, 2)

// Shapes of the small-batch ragged group kernel (ip_cksum / payload_cksum,
// nontemporal loads).
#define WC_RAGGED_SHAPE_LIST                                                   \
    WC_SHAPE(16, 2, 2)                                                         \
    WC_SHAPE(32, 4, 1)                                                         \
    WC_SHAPE(32, 3, 2)                                                         \
    WC_SHAPE(32, 2, 1)                                                         \
    WC_SHAPE(64, 2, 1)                                                         \
    WC_SHAPE(64, 4, 1)                                                         \
    WC_SHAPE(16, 6, 4)

// Shapes of the lean kernel (aligned strided batches, one pass per packet;
// wc_k_lean.hip): the planner's FULL shapes up to 576 B plus tuning
// neighbours for small packets.
#define WC_LEAN_SHAPE_LIST                                                     \
    WC_SHAPE(4, 1, 2)                                                      \
    WC_SHAPE(4, 1, 4)                                                      \
    WC_SHAPE(4, 2, 2)                                                      \
    WC_SHAPE(4, 2, 4)                                                      \
    WC_SHAPE(4, 3, 1)                                                      \
    WC_SHAPE(8, 1, 2)                                                      \
    WC_SHAPE(8, 1, 4)                                                      \
    WC_SHAPE(8, 1, 8)                                                      \
    WC_SHAPE(8, 2, 2)                                                      \
    WC_SHAPE(8, 2, 4)                                                      \
    WC_SHAPE(8, 3, 1)                                                      \
    WC_SHAPE(8, 3, 2)                                                      \
    WC_SHAPE(8, 6, 1)                                                      \
    WC_SHAPE(16, 1, 4)                                                     \
    WC_SHAPE(16, 2, 2)                                                     \
    WC_SHAPE(16, 2, 4)                                                     \
    WC_SHAPE(16, 3, 1)                                                     \
    WC_SHAPE(16, 3, 2)                                                     \
    WC_SHAPE(16, 6, 2)                                                     \
    WC_SHAPE(32, 1, 4)                                                     \
    WC_SHAPE(32, 2, 2)                                                     \
    WC_SHAPE(32, 2, 4)                                                     \
    WC_SHAPE(32, 3, 1)                                                     \
    WC_SHAPE(32, 3, 2)                                                     \
    WC_SHAPE(32, 4, 1)                                                     \
    WC_SHAPE(32, 4, 2)                                                     \
    WC_SHAPE(32, 18, 1)                                                    \
    WC_SHAPE(64, 1, 4)                                                     \
    WC_SHAPE(64, 2, 2)                                                     \
    WC_SHAPE(64, 3, 1)                                                     \
    WC_SHAPE(64, 4, 1)

namespace wc {

// Largest grid any launcher uses: gridDim.x * 256 threads must fit in a
// uint32 on AMD.  Every kernel strides over its work, so a capped grid stays
// correct (wc_cksum_api.cpp grid_for, the ragged launchers).
constexpr uint64_t kMaxGridBlocks = (1ull << 24) - 1;

// The grid of a tile kernel: one one-wave workgroup per tile of 64 frames.
inline int tile_grid(uint64_t n)
{
    const uint64_t tiles = (n + 63) / 64;
    return (int)(tiles > kMaxGridBlocks ? kMaxGridBlocks : tiles ? tiles : 1);
}

struct LaunchArgs {
    const void *base;
    uint64_t stride;
    uint32_t len;
    const uint64_t *offs;
    const uint16_t *lens;
    uint64_t n;
    uint16_t *out;
    uint64_t *bad;
    int kind;
    bool ragged; // offs/lens batch: flat kernel, or the ragged group kernel
    bool full;
    bool nontemporal;
    int tiles_per_wave; // flat kernel: 64-packet tiles each wave walks
    uint16_t *out_hdr;  // payload kind: also the IPv4 header checksums (or null)
    bool diag_noload;   // WC_DIAG_NOLOAD=1: timing-only flat build (wrong results)
    int variant = 0;    // WC_VARIANT: experimental kernel variants (A/B tuning)
    int seg_rows = 0;   // ragged: 0 = flat kernel, else k_cksum_seg with 2/4/8-row groups
    // k_cksum_seg: minimum chunk fill (in 64ths) for a tile's grouped path,
    // dense tiles | sparse tiles << 8 (65 = never)
    int grp_thr = 65 | (40 << 8);
    int grp_rows = 4; // k_cksum_seg grouped path: rows per ping-pong group (2, 4)
    int flat_pk = 1;  // flat kernel: 16-byte chunks per lane slot (1, or 2 = 32 B per lane)
    int gather = 1; // k_cksum_seg: gathered-stream path for tiles neither dense nor uniform
                    // (0 = flat path, 2 = for dense tiles too: tests)
};

struct Shape {
    int group;  // lanes per packet
    int cpl;    // 16-byte chunk loads per lane per pass
    int unroll; // packets per group per iteration
};

// Group-per-packet kernel: strided, or (a.ragged) the small-batch ragged
// variant over WC_RAGGED_SHAPE_LIST.
hipError_t launch_cksum(const LaunchArgs &a, const Shape &sh, int grid,
                        hipStream_t st);
// Aligned strided batches, one pass per packet (wc_k_lean.hip).
hipError_t launch_lean(const LaunchArgs &a, const Shape &sh, int grid, hipStream_t st);
// Ragged batches: a.seg_rows != 0 -> the segmented-prefix kernel (dense
// tiles; the rest take its flat path), else the chunk-balanced flat kernel
// (rows = 64-chunk rows per ping-pong group: 1, 2 or 4).
hipError_t launch_flat(const LaunchArgs &a, int rows, hipStream_t st);
// The standalone flat kernel (wc_k_flat.hip), behind launch_flat.
hipError_t launch_flat_kernel(const LaunchArgs &a, int rows, hipStream_t st);
hipError_t launch_synth(void *buf, uint64_t nbytes, uint64_t seed, int grid,
                        hipStream_t st);
hipError_t launch_sclk_probe(uint64_t *out, int n, uint64_t interval, hipStream_t st);
// RX verdicts of Ethernet frames [base + offs[i], + flens[i]) (wc_k_rx.hip);
// drops (optional) accumulates the frames the reference's RX path drops.
// mode: kRxEarly (parse, then stream only the checked frames) | kRxHdrT
// (transposed header loads) | kRxSkip (frames the parse rules out leave the
// stream); every mode gives the same verdicts.  `tally` (mapped host memory,
// kRxTallyWords words; ADAPT, with HT and without SKIP): every 64th tile
// stores gen << 16 | frames ruled out << 8 | frames, for the host's choice
// of EARLY or HT for the next launch.
constexpr int kRxEarly = 2, kRxHdrT = 4, kRxSkip = 8, kRxAdapt = 16;
constexpr uint32_t kRxTallyWords = 1024;
hipError_t launch_rx_verdict(const void *base, const uint64_t *offs, const uint16_t *flens,
                             uint64_t n, uint8_t *verdict, uint64_t *drops, bool nt,
                             hipStream_t st, int mode = 0, uint32_t *tally = nullptr,
                             uint32_t gen = 0, int max_grid = 0, void *rec = nullptr);
// `rec` (16-byte aligned, n struct wc_rx_record; the deliver calls): the
// DELIVER kernels also write every frame's delivery record.  They exist with
// transposed header loads and without SKIP only: kRxHdrT is implied and
// kRxSkip ignored.

// Stable compaction of verdict bytes (wc_k_rxsel.hip): list[0 .. *count) = the
// indices i < n, ascending, with (mask >> verdict[i]) & 1 (codes >= 32 never
// match); *count is stored.  Three launches on `st`: per-block match counts
// into `scratch` (rxsel_scratch_bytes(n) bytes, 4-byte aligned), one
// workgroup's exclusive scan of them, the scatter.  n <= 2^32.
uint64_t rxsel_scratch_bytes(uint64_t n);
hipError_t launch_rx_select(const uint8_t *verdict, uint64_t n, uint32_t mask, uint32_t *list,
                            uint64_t *count, void *scratch, hipStream_t st);

// RX socket demultiplex (wc_k_rxdemux.hip) behind a DELIVER launch over the
// same frames: sock[i] = the index of the socket frame i's record and address
// bytes select in `table` (a wc_rx_socktab_build blob of `ns` sockets, device
// memory), 0xFF for a delivered frame without one, 0xFE for rec[i].af == 0.
// With `list`: the delivered frames' indices grouped by socket, the unbound
// ones last, each group ascending, and start[256] (wc_cksum.h); `scratch`:
// rxdemux_scratch_bytes(n) bytes, 4-byte aligned.  One launch, or three with
// the list.  1 <= n <= 2^32, ns <= 254.
uint64_t rxdemux_scratch_bytes(uint64_t n);
hipError_t launch_rx_demux(const void *base, const uint64_t *offs, const void *rec, uint64_t n,
                           const void *table, uint32_t ns, uint8_t *sock, uint32_t *list,
                           uint64_t *start, void *scratch, hipStream_t st);

// RX replies (wc_k_rxreply.hip) behind an RX verdict / deliver (and demux)
// launch over the same frames.  Plan: action[i] = the enum wc_rx_reply_action
// code of frame i by the chain of wc_rx_reply.h over verdict[i], sock[i]
// (optional) and the engine table `eng` (struct wc_rx_engine, device memory,
// 4-byte aligned); reply_len[i] = the reply's frame length for a reply action,
// else 0.  One launch, no atomic.  1 <= n <= 2^32, slot_bytes <= 65535.
hipError_t launch_rx_reply_plan(const void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, const uint8_t *verdict, const uint8_t *sock,
                                const void *eng, uint32_t slot_bytes, uint8_t *action,
                                uint16_t *reply_len, bool nt, hipStream_t st);
// Build: reply j < MIN(*count, m) answers frame list[j] and is written at
// out_base + out_off[j] (at most slot_bytes bytes), out_len[j] its length; 0,
// and the slot untouched, for every other j < m and wherever the lengths
// derived again from the frame, the list index or the action byte do not
// allow a reply.  *built (zeroed by the caller on `st`) receives the number of
// non-zero lengths.  One launch of at most as many workgroups as the device's
// `cus` compute units hold at once (0: no cap), each striding over the replies;
// m >= 1.
hipError_t launch_rx_reply_build(const void *base, const uint64_t *offs, const uint16_t *flens,
                                 uint64_t n, const uint8_t *action, const uint32_t *list,
                                 const uint64_t *count, const void *eng, void *out_base,
                                 const uint64_t *out_off, uint32_t m, uint32_t slot_bytes,
                                 const uint16_t *ip_id, uint16_t *out_len, uint64_t *built,
                                 int cus, hipStream_t st);

// RX neighbours (wc_k_rxneigh.hip) behind a reply plan launch over the same
// frames.  Plan: nact[i] = the enum wc_rx_neigh_action code of frame i by the
// chain of wc_rx_neigh.h over action[i] (the reply plan's) and the engine table
// `eng` (4-byte aligned).  One launch, no atomic.  1 <= n <= 2^32.
hipError_t launch_rx_neigh_plan(const void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, const uint8_t *action, const void *eng, uint8_t *nact,
                                hipStream_t st);
// Updates: upd[j] (struct wc_neigh_update, 4-byte aligned) = the record of
// frame list[j] for j < MIN(*count, m), all zero for every other j < m and
// wherever the index, the code byte or the frame length allow no record.
// Build: as launch_rx_reply_build, for the is-at and advertisement frames.
// Each is one launch of at most as many workgroups as the device's `cus`
// compute units hold at once (0: no cap); m >= 1.
hipError_t launch_rx_neigh_updates(const void *base, const uint64_t *offs, const uint16_t *flens,
                                   uint64_t n, const uint8_t *nact, const uint32_t *list,
                                   const uint64_t *count, uint32_t m, void *upd, int cus,
                                   hipStream_t st);
hipError_t launch_rx_neigh_build(const void *base, const uint64_t *offs, const uint16_t *flens,
                                 uint64_t n, const uint8_t *nact, const uint32_t *list,
                                 const uint64_t *count, const void *eng, void *out_base,
                                 const uint64_t *out_off, uint32_t m, uint32_t slot_bytes,
                                 uint16_t *out_len, uint64_t *built, int cus, hipStream_t st);

// RX drain (wc_k_rxdrain.hip): for 0 <= n <= kRxDrainSmall frames, every output
// array of launch_rx_verdict (with `rec`), launch_rx_demux, launch_rx_reply_plan
// (sock given) and launch_rx_neigh_plan with their four lists (launch_rx_select
// over the action and nact bytes), byte for byte, in two launches: one wave per
// 64-frame tile for the six per-frame arrays, then one workgroup for the lists,
// the 256 start entries and the three counts.  n = 0: the second launch alone,
// which then reads no array.  Every pointer but drops is given; rec 16-byte,
// table and eng 4-byte aligned; ns <= 254.
constexpr uint32_t kRxDrainSmall = 4096; // WC_RX_DRAIN_SMALL
struct RxDrainArrays {
    uint8_t *verdict;
    void *rec;
    uint64_t *drops;
    uint8_t *sock;
    uint32_t *list;
    uint64_t *start;
    uint8_t *action;
    uint16_t *reply_len;
    uint32_t *rlist;
    uint64_t *rcount;
    uint8_t *nact;
    uint32_t *nrlist;
    uint64_t *nrcount;
    uint32_t *ulist;
    uint64_t *ucount;
};
hipError_t launch_rx_drain(const void *base, const uint64_t *offs, const uint16_t *flens,
                           uint64_t n, const void *table, uint32_t ns, const void *eng,
                           uint32_t slot_bytes, const RxDrainArrays &o, bool nt, hipStream_t st);

// TX seal of Ethernet frames [base + offs[i], + flens[i]) (wc_k_tx.hip): both
// checksums computed with their fields taken as 0 and stored raw into the
// frame, status[i] its enum wc_tx_status code; out_ip / out_udp (optional)
// receive the values, 0 where none is computed; errors (optional) accumulates
// the WC_TX_IS_ERROR frames.  flags: kTxZeroUdp (udp->cksum = 0, no payload
// byte read) | kTxNoStore (compute only: no frame byte is written).
constexpr uint32_t kTxZeroUdp = 1, kTxNoStore = 2;
hipError_t launch_tx_seal(void *base, const uint64_t *offs, const uint16_t *flens, uint64_t n,
                          uint32_t flags, uint8_t *status, uint16_t *out_ip, uint16_t *out_udp,
                          uint64_t *errors, bool nt, hipStream_t st);

// TX build (wc_k_txbuild.hip): frame i starts at base + offs[i], its payload
// already at + 14 + hl + 8; the headers in front of it are synthesised from
// desc[i] (struct wc_tx_desc, 8-byte aligned), the socket table (ns struct
// wc_tx_sock) and the destination table (ndst struct wc_tx_dst) and stored,
// both checksums included.  frame_len[i] = the built frame's length (0 for an
// error status), status[i] its enum wc_tx_status code; out_ip / out_udp
// (optional) the two values; errors (optional) accumulates the error frames.
// flags: kTxZeroUdp | kTxNoStore, as the seal's.
hipError_t launch_tx_build(void *base, const uint64_t *offs, const void *desc, uint64_t n,
                           const void *socks, uint32_t ns, const void *dsts, uint32_t ndst,
                           uint32_t slot_bytes, uint32_t flags, uint16_t *frame_len,
                           uint8_t *status, uint16_t *out_ip, uint16_t *out_udp, uint64_t *errors,
                           bool nt, hipStream_t st);

// TX neighbours (wc_k_txneigh.hip; layout and steps in wc_tx_neigh.h).  Every
// launch is at most as many workgroups as the device's `cus` compute units hold
// at once (0: no cap), each striding.
// Init: the table's tab_bytes(cap) bytes zeroed, magic and cap written.
hipError_t launch_neigh_tab_init(void *tab, uint32_t cap, int cus, hipStream_t st);
// Apply: records j < MIN(*count, m) of upd (struct wc_neigh_update, 4-byte
// aligned) into the table, as if in order; scratch: m words; *dropped (optional)
// accumulates, one atomic per workgroup.  Two launches; 1 <= m <= 2^31.
hipError_t launch_neigh_apply(void *tab, const void *upd, const uint64_t *count, uint32_t m,
                              uint64_t *dropped, void *scratch, int cus, hipStream_t st);
// Resolve: state[k] and dsts[k].dmac for k < ndst (1 <= ndst <= 65536) from the
// table and afs[k]; scratch: tx_resolve_set_bytes(ndst) bytes, 4-byte aligned,
// zeroed here.  A memset and two launches.
uint64_t tx_resolve_set_bytes(uint32_t ndst);
hipError_t launch_tx_resolve(const void *tab, void *dsts, const uint8_t *afs, uint32_t ndst,
                             uint8_t *state, void *scratch, int cus, hipStream_t st);
// Hold plan: hold[i] = the enum wc_tx_hold code of frame i; one launch, n >= 1.
hipError_t launch_tx_hold_plan(const void *desc, uint64_t n, const void *socks, uint32_t ns,
                               const uint8_t *state, const uint8_t *afs, uint32_t ndst,
                               uint8_t *hold, int cus, hipStream_t st);
// Solicit build: as launch_rx_neigh_build, for the who-has and solicitation
// frames of destinations list[j]; m >= 1, ndst >= 1.
hipError_t launch_tx_solicit_build(const void *dsts, const uint8_t *afs, uint32_t ndst,
                                   const uint32_t *list, const uint64_t *count, const void *eng,
                                   void *out_base, const uint64_t *out_off, uint32_t m,
                                   uint32_t slot_bytes, uint16_t *out_len, uint64_t *built, int cus,
                                   hipStream_t st);

// TX pump (wc_k_txpump.hip, wc_k_txbuild.hip; the gate and the destination
// steps in wc_tx_pump.h).  Plan: for 0 <= n <= tp::kSmall frames, 0 <= ndst <=
// tp::kSmallDst destinations and 0 <= m <= tp::kSmallDst solicitation slots,
// every output of launch_tx_resolve,
// launch_tx_hold_plan (both with their launch_rx_select lists) and
// launch_tx_solicit_build, byte for byte, from one workgroup; the three counts
// are always written.  An empty side's pointers are not looked at (m = 0: none
// of the solicitation side but sol_built).
struct TxPumpArrays {
    uint8_t *state;
    uint32_t *miss_list;
    uint64_t *miss_count;
    uint8_t *hold;
    uint32_t *held_list;
    uint64_t *held_count;
    uint16_t *sol_len;
    uint64_t *sol_built;
};
hipError_t launch_tx_pump_plan(const void *tab, void *dsts, const uint8_t *afs, uint32_t ndst,
                               const void *desc, uint32_t n, const void *socks, uint32_t ns,
                               const void *eng, void *sol_base, const uint64_t *sol_off, uint32_t m,
                               uint32_t sol_slot_bytes, const TxPumpArrays &o, hipStream_t st);
// Gated build: launch_tx_build's frame for any n >= 1, with hold[i] (enum
// wc_tx_hold) deciding per frame by tp::gate: only a READY frame is built.
// flags: kTxZeroUdp or 0.
hipError_t launch_tx_build_gated(void *base, const uint64_t *offs, const void *desc, uint64_t n,
                                 const void *socks, uint32_t ns, const void *dsts, uint32_t ndst,
                                 uint32_t slot_bytes, uint32_t flags, const uint8_t *hold,
                                 uint16_t *frame_len, uint8_t *status, uint16_t *out_ip,
                                 uint16_t *out_udp, uint64_t *errors, bool nt, hipStream_t st);

// RX answer (wc_k_rxanswer.hip): for at most ra::kSmall entries in each of the
// three lists, every output of launch_rx_reply_build, launch_rx_neigh_updates,
// launch_rx_neigh_build and launch_neigh_apply, from two launches and with no
// memset in front: launch_rx_answer_frames, one grid whose workgroups are
// split between the three list kernels' bodies (wc_rx_answer.h; it writes
// neither built count, and with n = 0 zero lengths and zero records), and
// launch_rx_answer_apply, one workgroup that counts the stored lengths into
// *r_built and *n_built (written, not accumulated) and, where tab is given and
// u_m > 0, applies the records with its entry indices in LDS.  A part with m =
// 0 has none of its pointers looked at but its built count.
struct RxAnswerArgs {
    const uint8_t *base;
    const uint64_t *offs;
    const uint16_t *flens;
    uint64_t n;
    const uint32_t *eng;
    uint32_t slot_bytes;
    const uint8_t *action;
    const uint32_t *rlist;
    const uint64_t *rcount;
    const uint8_t *nact;
    const uint32_t *nrlist;
    const uint64_t *nrcount;
    const uint32_t *ulist;
    const uint64_t *ucount;
    uint8_t *r_out_base;
    const uint64_t *r_out_off;
    uint32_t r_m;
    const uint16_t *ip_id;
    uint16_t *r_out_len;
    uint64_t *r_built;
    uint8_t *n_out_base;
    const uint64_t *n_out_off;
    uint32_t n_m;
    uint16_t *n_out_len;
    uint64_t *n_built;
    uint32_t u_m;
    uint32_t *upd;
    uint32_t *tab;
    uint64_t *dropped;
};
// (no launch where all three m are 0)
hipError_t launch_rx_answer_frames(const RxAnswerArgs &a, int cus, hipStream_t st);
hipError_t launch_rx_answer_apply(const RxAnswerArgs &a, hipStream_t st);

// RX echo (wc_k_rxecho.hip; the map and the copy in wc_rx_echo.h): the
// delivered frames of the switched-on sockets as a TX batch -- all m entries
// of desc / dsts / af / status (and src / tx_off where given), *count, the
// payloads in copy mode (out_base / out_off given, tx_off NULL) -- from one
// launch of re::grid_of(m) one-wave workgroups for any n <= 2^32 and m <=
// re::kMax.  n = 0 or ns = 0: no RX pointer is looked at.
struct RxEchoArgs {
    const uint8_t *base;
    const uint64_t *offs;
    const uint16_t *flens;
    uint64_t n;
    const void *rec;
    const uint32_t *list;
    const uint64_t *start;
    const uint16_t *map;
    uint32_t ns;
    const uint16_t *ip_id;
    uint8_t *out_base;
    const uint64_t *out_off;
    uint32_t out_slot_bytes;
    uint32_t m;
    uint32_t *desc;
    uint32_t *dsts;
    uint8_t *af;
    uint8_t *status;
    uint32_t *src;
    uint64_t *tx_off;
    uint64_t *count;
    uint64_t *skipped;
};
hipError_t launch_rx_echo(const RxEchoArgs &a, hipStream_t st);

// Resident small-batch server (wc_k_serve.hip).  Host-mapped pinned memory:
// one record per packet, written by the host (seq last), polled / read by the
// server's waves; one result slot per packet, written by the GPU in one
// 8-byte store.  Requests are numbered by seq (never 0 after the first).
constexpr uint32_t kSrvMaxPkts = 1024;  // packets per request
constexpr uint32_t kSrvMaxBytes = 4064; // bytes one packet (frame) may span
constexpr uint32_t kSrvKindRx = 2;      // record kind beside WC_KIND_IP / _PAYLOAD
// Fused TX record: payload_cksum(pkt, len) | ip_cksum(pkt, ip4_hl) << 16 (0
// for IPv6), the two checksums mk_ip4_hdr + udp_tx compute (ip4.c:184-186,
// udp.c:209-213).
constexpr uint32_t kSrvKindFused = 3;
constexpr int kSrvAddrBits = 48;        // the packet count rides above the address
struct alignas(16) SrvRec {
    uint64_t addr; // device address of the packet / frame (< 2^48) | n << 48
    uint32_t info; // len | kind << 16 | stop << 24
    uint32_t seq;  // request number, stored last
};
struct alignas(8) SrvRes {
    uint32_t value; // checksum or RX verdict
    uint32_t seq;   // the request it answers
};
// d_hb: the host's heartbeat word (the latest request number, written before
// every request's records): a wave leaves on its own only after idle_ticks in
// which the heartbeat did not move, so the grid drains as a whole.
hipError_t launch_serve(const SrvRec *d_recs, SrvRes *d_res, const uint32_t *d_hb, uint32_t seq0,
                        int waves, uint64_t idle_ticks, hipStream_t st);

} // namespace wc
