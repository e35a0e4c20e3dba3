/*
 * wc_cksum.h -- C ABI of the MI355X (gfx950) Internet / UDP checksum library
 * (libwccksum.so).  Plain C types only; every device-side pointer is a HIP
 * device (or mapped pinned host) address, every `stream` is a hipStream_t
 * passed as void* (NULL = the legacy default stream).
 *
 * Drop-in boundary.  The reference exposes exactly two checksum entry points,
 * declared at /root/reference/lib/src/in_cksum.h:32-36 and defined at
 * /root/reference/lib/src/in_cksum.c:133-167:
 *
 *     uint16_t ip_cksum(const void *buf, uint16_t len);
 *     uint16_t payload_cksum(const void *buf, uint16_t len);
 *
 * This library exports both under the same names and with the same semantics
 * (bit-identical results, no error channel, result stored raw into the
 * packet), computed on the GPU.  Around them it adds the batch entry points
 * the reference's per-packet loops would call at their natural batch points
 * (w_tx's sq_foreach, backend_netmap.c:348-358, and the RX ring drain,
 * backend_netmap.c:379-391); see INTEGRATION.md.
 *
 * Return convention of the int-returning functions: 0 on success, a negative
 * WC_E* code on a caller error, or -(int)hipError_t on a HIP runtime error.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Which reference function each packet is checksummed with. */
enum wc_cksum_kind {
    WC_CKSUM_IP = 0,      /* ip_cksum(buf, len)       in_cksum.c:133-137 */
    WC_CKSUM_PAYLOAD = 1, /* payload_cksum(buf, len)  in_cksum.c:140-167 */
};

/* Library error codes (HIP errors are returned as -(int)hipError_t, which
 * never collides with these). */
#define WC_OK 0
#define WC_EINVAL (-10001)   /* bad argument (NULL pointer, bad kind, ...) */
#define WC_ENODEV (-10002)   /* no usable gfx950 device */
#define WC_ENOMEM (-10003)   /* scratch / staging allocation failed */
#define WC_ECOMM (-10004)    /* RCCL unavailable or a collective failed */

/* --- drop-in scalar entry points (reference in_cksum.h:32-36) ------------ */

/* Same contract as the reference: `buf` is host memory owned by the caller
 * (a netmap slot or w_iov buffer), read only; the return value is the
 * checksum as a native uint16 whose in-memory bytes are the network-order
 * checksum.  There is no error channel -- like the reference's ensure()/die()
 * (util.h:280-340) an unusable GPU aborts the process with a message. */
uint16_t ip_cksum(const void *buf, uint16_t len);
uint16_t payload_cksum(const void *buf, uint16_t len);

/* --- device-resident batch entry points ---------------------------------- */

/* Packet i occupies [base + i*stride, base + i*stride + len).  Any alignment
 * and any stride (including stride < len, overlapping) is accepted.
 * out[i] receives the checksum of packet i (device memory, n entries). */
int wc_cksum_strided(const void *d_base, uint64_t stride, uint16_t len,
                     uint64_t n, uint16_t *d_out, int kind, void *stream);

/* Packet i occupies [base + d_off[i], base + d_off[i] + d_len[i]) (d_off and
 * d_len are device arrays of n entries).  Any alignment is accepted. */
int wc_cksum_ragged(const void *d_base, const uint64_t *d_off,
                    const uint16_t *d_len, uint64_t n, uint16_t *d_out,
                    int kind, void *stream);

/* RX-side verification (udp.c:132-139, ip4.c:110-115): like the batch calls
 * above, and additionally counts the packets whose checksum is not 0 into
 * *d_bad (a device uint64, accumulated, not reset).  d_out may be NULL. */
int wc_verify_strided(const void *d_base, uint64_t stride, uint16_t len,
                      uint64_t n, uint16_t *d_out, uint64_t *d_bad, int kind,
                      void *stream);
int wc_verify_ragged(const void *d_base, const uint64_t *d_off,
                     const uint16_t *d_len, uint64_t n, uint16_t *d_out,
                     uint64_t *d_bad, int kind, void *stream);

/* Fused IP + UDP pass over IP packets (each at its IP header, len = IP
 * header + UDP length, as payload_cksum takes them): d_out_payload[i] =
 * payload_cksum(pkt, len) and d_out_ip_hdr[i] = ip_cksum(pkt, ip4_hl(pkt[0]))
 * -- the IPv4 header checksum mk_ip4_hdr / ip4_rx compute (ip4.c:184-186,
 * 110-115) -- or 0 for an IPv6 packet, which has no header checksum
 * (ip6.c:83-113).  One read of the packet bytes for both.  An IPv4 header
 * (hl bytes, options included) must lie inside the caller's device buffer
 * even where len is shorter: its checksum is defined whatever len is, and
 * both calls read it whole.  len < hl itself is outside payload_cksum's
 * defined inputs (the reference's len - hl wraps to ~4 GiB, in_cksum.c:164):
 * d_out_payload[i] is then unspecified. */
int wc_cksum_ip_udp_strided(const void *d_base, uint64_t stride, uint16_t len,
                            uint64_t n, uint16_t *d_out_ip_hdr,
                            uint16_t *d_out_payload, void *stream);
int wc_cksum_ip_udp_ragged(const void *d_base, const uint64_t *d_off,
                           const uint16_t *d_len, uint64_t n, uint16_t *d_out_ip_hdr,
                           uint16_t *d_out_payload, void *stream);

/* --- RX verdict: the reference's RX checks, decided on the device -------- */

/* What the reference's RX path decides for one Ethernet frame from its
 * checksums and header format: eth_rx (eth.c:75-86) -> ip4_rx
 * (ip4.c:95-138) / ip6_rx (ip6.c:91-111) -> udp_rx (udp.c:99-139).  The
 * checks run in the reference's order; the first that fails names the code.
 * Engine state -- MAC and IP address filters (eth.c:65-73, ip4.c:103-108,
 * ip6.c:98-103), bound sockets -- is not part of the verdict. */
enum wc_rx_verdict {
    WC_RX_OK = 0,            /* UDP, checksum verified (udp.c:134): deliver */
    WC_RX_OK_NO_CKSUM = 1,   /* UDP checksum field 0: accepted unverified (udp.c:132) */
    WC_RX_BAD_IP_CKSUM = 2,  /* ip_cksum(ip, hl) != 0 (ip4.c:110-115): drop */
    WC_RX_BAD_UDP_CKSUM = 3, /* payload_cksum(ip, udp_len + hl) != 0 (udp.c:134-139): drop */
    WC_RX_SHORT = 4,         /* IP payload shorter than a UDP header (udp.c:123-126): drop */
    WC_RX_FRAGMENT = 5,      /* IPv4 fragment offset != 0 (ip4.c:123-127): drop */
    WC_RX_BAD_VERSION = 6,   /* version nibble != the EtherType's (ip4.c:95-98, ip6.c:91-95): drop */
    WC_RX_NOT_UDP = 7,       /* IPv4 / IPv6, another protocol (ICMP, ...): the host's (ip4.c:129-137) */
    WC_RX_NOT_IP = 8,        /* EtherType neither IPv4 nor IPv6 (ARP, ...): the host's (eth.c:75-86) */
    WC_RX_TRUNCATED = 9,     /* a byte the reference reads lies past the frame: drop */
};
#define WC_RX_IS_DROP(v) \
    ((v) != WC_RX_OK && (v) != WC_RX_OK_NO_CKSUM && (v) != WC_RX_NOT_UDP && (v) != WC_RX_NOT_IP)

/* Frame i is the Ethernet frame [d_base + d_off[i], + d_frame_len[i]) -- a
 * netmap slot buffer and its slot length (backend_netmap.c:379-391), or any
 * batch of frames; no header is parsed on the host.  d_verdict[i] receives
 * its enum wc_rx_verdict code (uint8); *d_drops (device uint64, optional,
 * accumulated) counts the frames whose code is a drop (WC_RX_IS_DROP).  No
 * byte outside a frame is read: what the reference would read past the frame
 * (its neighbouring buffers) yields WC_RX_TRUNCATED. */
int wc_rx_verdict_ragged(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                         uint64_t n, uint8_t *d_verdict, uint64_t *d_drops, void *stream);

/* Host-memory frames (the netmap buffer area w->mem, ideally registered with
 * wc_host_register): synchronous; *h_drops (optional) = the drop count. */
int wc_rx_verdict_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                       const uint16_t *h_frame_len, uint64_t n, uint8_t *h_verdict,
                       uint64_t *h_drops);

/* --- RX delivery: per-frame UDP records and index lists ------------------ */

/* What udp_rx puts into the w_iov of an accepted frame (udp.c:101-142,
 * 163-165), 16 bytes, little-endian, all offsets from the frame's first byte.
 * All-zero (af == 0) for every frame whose verdict is not WC_RX_OK /
 * WC_RX_OK_NO_CKSUM. */
struct wc_rx_record {
    uint16_t data_off; /* i->buf: 14 + hl + 8                                  */
    uint16_t data_len; /* i->len: (uint16_t)(MIN(udp->len, ip_plen) - 8), as the
                          reference computes it, wrap included; for OK_NO_CKSUM
                          the reference never holds it against the slot length,
                          and neither does the record                          */
    uint16_t sport;    /* udp->sport as stored (network-order bytes), udp.c:141 */
    uint16_t dport;    /* udp->dport as stored, udp.c:142                       */
    uint8_t af;        /* 4 or 6                                               */
    uint8_t tos;       /* i->flags: ip4->tos, or ip6_tos(vtcecnfl) (ip6.h:77-81)*/
    uint8_t ttl;       /* ip4->ttl / ip6->hlim                                 */
    uint8_t hl;        /* ip_hdr_len: ip4_hl(vhl) or 40                        */
    uint16_t src_off;  /* ip->src: 14 + 12 (IPv4), 14 + 8 (IPv6)               */
    uint16_t dst_off;  /* ip->dst: 14 + 16 (IPv4), 14 + 24 (IPv6)              */
};

/* Sets of verdict classes, for wc_rx_select. */
#define WC_RX_MASK(v) (1u << (v))
#define WC_RX_MASK_DELIVER (WC_RX_MASK(WC_RX_OK) | WC_RX_MASK(WC_RX_OK_NO_CKSUM))
#define WC_RX_MASK_HOST    (WC_RX_MASK(WC_RX_NOT_UDP) | WC_RX_MASK(WC_RX_NOT_IP))

/* Bytes of d_scratch the two calls below need for n frames (pure arithmetic,
 * no GPU; 0 for n = 0, never decreasing in n).  The scratch is the caller's
 * (device memory, 4-byte aligned, one per call in flight): the device calls
 * take no library lock and may run concurrently on several streams. */
uint64_t wc_rx_select_scratch(uint64_t n);

/* d_list[0 .. *d_count) = the indices i, ascending, of the frames with
 * (mask >> d_verdict[i]) & 1 (codes >= 32 never match); *d_count (a device
 * uint64) is written, not accumulated; entries past *d_count are left as they
 * were, so d_list needs as many entries as can match (n always suffices).
 * n = 0 is WC_OK, writes *d_count = 0 where d_count is given, and looks at
 * no other pointer (all may be NULL); n > 2^32 is WC_EINVAL.  Asynchronous on `stream`:
 * three short launches, no atomic and no wait between workgroups. */
int wc_rx_select(const uint8_t *d_verdict, uint64_t n, uint32_t mask,
                 uint32_t *d_list, uint64_t *d_count, void *d_scratch, void *stream);

/* wc_rx_verdict_ragged -- the same verdicts and *d_drops for the same frames
 * -- plus d_rec[i] for every frame (d_rec 16-byte aligned, as any device
 * allocation is), and, with d_list non-NULL,
 * wc_rx_select(d_verdict, n, WC_RX_MASK_DELIVER, ...) behind it on the same
 * stream.  d_list and d_count go together (both or neither): that is checked
 * first, for every n, so a count without a list is WC_EINVAL for n = 0 too
 * (unlike wc_rx_select, which for n = 0 takes a lone count).  Then n = 0 is
 * WC_OK, writes *d_count = 0 if the pair is given, and looks at no other
 * pointer.  d_scratch may be NULL only when d_list is.  No header is parsed on the host, and no byte
 * outside a frame is read: every field of a record lies in bytes the checks
 * before WC_RX_OK / WC_RX_OK_NO_CKSUM have placed inside the frame. */
int wc_rx_deliver_ragged(const void *d_base, const uint64_t *d_off,
                         const uint16_t *d_frame_len, uint64_t n, uint8_t *d_verdict,
                         struct wc_rx_record *d_rec, uint32_t *d_list, uint64_t *d_count,
                         uint64_t *d_drops, void *d_scratch, void *stream);

/* Host-memory frames, by the paths of wc_rx_verdict_host except the resident
 * server (a zero-copy launch, in-place streaming or the pipeline);
 * synchronous.  h_list / *h_count (optional, both or neither -- checked
 * first, as above, for n = 0 too) = the WC_RX_MASK_DELIVER list, built by the
 * calling thread from the verdict bytes; *h_drops (optional) = the drop count.
 * n = 0 is WC_OK and writes 0 to whichever counts are given. */
int wc_rx_deliver_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                       const uint16_t *h_frame_len, uint64_t n, uint8_t *h_verdict,
                       struct wc_rx_record *h_rec, uint32_t *h_list, uint64_t *h_count,
                       uint64_t *h_drops);

/* --- RX socket demultiplex: per-frame socket ids, per-socket lists -------- */

/* What udp_rx does next with a delivered frame (udp.c:141-156, 174): it looks
 * up the socket of local = (af, ip->dst, udp->dport) and remote = (af,
 * ip->src, udp->sport) -- w_get_sock(w, &local, &remote), then
 * w_get_sock(w, &local, 0) (backend_netmap.c:481-490), both exact compares
 * (warpcore.c:644-677) -- and appends the iov to that socket's queue, or
 * sends an ICMP unreachable when there is none.  The lookup and the grouping
 * run on the device; the engine's sockets are handed over as a small table. */
#define WC_RX_DEMUX_MAX_SOCKS 254
#define WC_RX_SOCK_NONE    0xFE  /* frame not delivered (record af == 0)            */
#define WC_RX_SOCK_UNBOUND 0xFF  /* delivered, no socket: the host's ICMP unreachable
                                    decision (udp.c:147-155)                        */
struct wc_rx_sock {              /* 40 bytes; one bound or connected w_sock         */
    uint8_t  af;                 /* 4 or 6                                          */
    uint8_t  connected;          /* 0: bound only (remote ignored); 1: four-tuple   */
    uint16_t lport, rport;       /* as stored in the UDP header (like record ports) */
    uint16_t pad;                /* ignored                                         */
    uint8_t  laddr[16], raddr[16]; /* af 4: bytes 0..3 count, 4..15 ignored         */
};

/* The socket table: an opaque, position-independent blob of
 * wc_rx_socktab_bytes(ns) bytes (never decreasing in ns) that
 * wc_rx_socktab_build writes into h_tab (4-byte aligned) from socks[0 .. ns)
 * -- an open-addressing hash table holding every socket's whole tuple and its
 * index, so a probe ends on an exact compare; the same input gives the same
 * bytes.  Pure host arithmetic: no GPU, no library state.  The caller copies
 * the blob to the device for wc_rx_demux, again whenever w_bind / w_connect /
 * w_close change the sockets.  WC_EINVAL: ns > WC_RX_DEMUX_MAX_SOCKS, a NULL
 * pointer (socks may be NULL for ns = 0), an af other than 4 / 6, connected
 * other than 0 / 1, or two sockets with the same tuple once the ignored bytes
 * are dropped (the reference's hash cannot hold such a pair either). */
uint64_t wc_rx_socktab_bytes(uint32_t ns);
int      wc_rx_socktab_build(const struct wc_rx_sock *socks, uint32_t ns, void *h_tab);

/* The table's own lookup on the host, by the reference's two steps: the index
 * of the connected socket with exactly this local and remote pair, else of
 * the socket bound to the local pair, else WC_RX_SOCK_UNBOUND (also for an af
 * other than 4 / 6 or a blob that build did not write).  Addresses as
 * struct wc_rx_sock holds them (af 4: 4 bytes are read), ports as stored. */
uint8_t  wc_rx_socktab_lookup(const void *h_tab, uint8_t af, const uint8_t *laddr, uint16_t lport,
                              const uint8_t *raddr, uint16_t rport);

/* Bytes of d_scratch wc_rx_demux needs for n frames with a list (pure
 * arithmetic, no GPU; 0 for n = 0, never decreasing in n): per-block counts
 * for the most classes a table can have. */
uint64_t wc_rx_demux_scratch(uint64_t n);

/* Behind a wc_rx_deliver_ragged of the same frames on the same stream (it
 * reads d_rec, not the verdicts or frame lengths): d_sock[i] = the index in
 * the table (d_tab: the blob in device memory, built for ns sockets) of frame
 * i's socket, WC_RX_SOCK_UNBOUND, or WC_RX_SOCK_NONE where d_rec[i].af == 0.
 * With d_list / d_start (both or neither: checked first, for every n):
 * d_list = the delivered frames' indices grouped by socket 0 .. ns - 1, the
 * unbound frames last, each group in ascending ring order (as sq_insert_tail
 * queues them); it needs as many entries as frames can be delivered (n always
 * suffices), entries past the total are left as they were.  d_start has 256
 * entries whatever ns is: socket s's run is d_list[d_start[s] .. d_start[s+1])
 * for s < 254 (empty for s >= ns), the unbound run [d_start[254],
 * d_start[255]), and d_start[255] = the number of delivered frames.  n = 0 is
 * WC_OK, writes an all-zero d_start if given and looks at no other pointer.
 * WC_EINVAL: n > 2^32, ns > 254, a NULL d_base / d_off / d_rec / d_tab /
 * d_sock, d_rec not 16-byte or d_tab not 4-byte aligned, a list without a
 * 4-byte-aligned d_scratch (the caller's, one per call in flight; it may be
 * NULL without a list).  The address bytes are read as the aligned 16-byte
 * chunks that overlap them; they lie inside the frame by the checks that gave
 * the frame its record.  Asynchronous on `stream`: one launch, three with the
 * list; no library lock, no atomic, no wait between workgroups, and the same
 * input gives the same output. */
int wc_rx_demux(const void *d_base, const uint64_t *d_off, const struct wc_rx_record *d_rec,
                uint64_t n, const void *d_tab, uint32_t ns, uint8_t *d_sock,
                uint32_t *d_list, uint64_t *d_start, void *d_scratch, void *stream);

/* wc_rx_deliver_host's verdicts, records and drop count for the same frames,
 * plus h_sock and (optional, both or neither -- checked first) h_list /
 * h_start as above, built by the calling thread from the h_sock bytes.
 * h_tab: the blob in host memory, as wc_rx_socktab_build wrote it for ns
 * sockets (WC_EINVAL otherwise); the library stages it once per call.
 * Synchronous; never the resident server.  n = 0 is WC_OK and writes zeros to
 * h_start and *h_drops where given. */
int wc_rx_demux_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                     const uint16_t *h_frame_len, uint64_t n, const void *h_tab, uint32_t ns,
                     uint8_t *h_verdict, struct wc_rx_record *h_rec, uint8_t *h_sock,
                     uint32_t *h_list, uint64_t *h_start, uint64_t *h_drops);

/* --- TX seal: both checksums computed and stored in the frames ----------- */

/* What mk_ip4_hdr and udp_tx do to a frame (ip4.c:184-186, udp.c:209-213),
 * for a batch of Ethernet frames: the device parses each frame, computes
 * ip_cksum(ip, hl) with header bytes 10..11 taken as 0 (IPv4; options
 * included) and payload_cksum(ip, hl + udp_len) with udp->cksum taken as 0,
 * and stores both raw (native uint16, any address parity) into the frame.
 * Whatever the two fields hold on entry does not matter, so the call is
 * idempotent; a computed UDP checksum of 0 is stored as 0 (udp.c:213).  The
 * checks run in the order of the RX chain above; the first that fails names
 * the code.  A sealed frame is one wc_rx_verdict_* accepts. */
enum wc_tx_status {
    WC_TX_SEALED = 0,          /* UDP over IPv4 / IPv6: every checksum field the frame has is written */
    WC_TX_SEALED_ZERO_UDP = 1, /* WC_TX_ZERO_UDP_CKSUM: IPv4 header checksum written, udp->cksum written 0 */
    WC_TX_IP_ONLY = 2,         /* IPv4, not UDP or a fragment (offset != 0): header checksum written, nothing else */
    WC_TX_NOT_UDP = 3,         /* IPv6, another next header: untouched (ICMPv6 is the host's, icmp6.c:73) */
    WC_TX_NOT_IP = 4,          /* EtherType neither IPv4 nor IPv6 (ARP): untouched */
    WC_TX_BAD_VERSION = 5,     /* version nibble != the EtherType's: untouched */
    WC_TX_MALFORMED = 6,       /* IHL < 5, IP payload < 8, or MIN(udp->len, ip_plen) < 8: untouched */
    WC_TX_TRUNCATED = 7,       /* a byte that would be read or written lies past the frame: untouched */
};
#define WC_TX_IS_ERROR(s) ((s) >= WC_TX_BAD_VERSION)

#define WC_TX_ZERO_UDP_CKSUM 1u /* the socket's enable_udp_zero_checksums (udp.c:212): no payload byte is read */
#define WC_TX_NO_STORE 2u       /* compute only: frames untouched, both d_out arrays required */

/* Frame i is the Ethernet frame [d_base + d_off[i], + d_frame_len[i]); the
 * frames of one call must not overlap (they may share 16-byte chunks and
 * cache lines).  d_status[i] receives its enum wc_tx_status code (uint8);
 * d_out_ip_hdr / d_out_udp (optional) the two values, 0 where none is
 * computed; *d_errors (device uint64, optional, accumulated) counts the
 * WC_TX_IS_ERROR frames.  "Untouched" means no byte of the frame is written;
 * for every status no byte outside the frame is read or written, and no byte
 * of the frame but the two fields is ever written.  Unknown flag bits, and
 * WC_TX_NO_STORE without both out arrays, are WC_EINVAL.  One asynchronous
 * launch on `stream`. */
int wc_tx_seal_ragged(void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                      uint64_t n, uint32_t flags, uint8_t *d_status,
                      uint16_t *d_out_ip_hdr, uint16_t *d_out_udp,
                      uint64_t *d_errors, void *stream);

/* Host-memory frames (a w_iov_sq's buffers in w->mem, ideally registered with
 * wc_host_register), every frame inside [h_base, h_base + h_bytes) (WC_EINVAL
 * otherwise): the device computes over the host paths of wc_cksum_host (a
 * zero-copy launch, in-place streaming or the pipeline; never the resident
 * server) and the calling thread makes the stores.  Synchronous; *h_errors
 * (optional) = the WC_TX_IS_ERROR count.  WC_TX_NO_STORE is WC_EINVAL here. */
int wc_tx_seal_host(void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                    const uint16_t *h_frame_len, uint64_t n, uint32_t flags,
                    uint8_t *h_status, uint64_t *h_errors);

/* --- TX build: Ethernet / IP / UDP headers written from a socket table ---- */

/* The per-iov body of udp_tx (udp.c:189-220): mk_ip4_hdr / mk_ip6_hdr
 * (ip4.c:153-189, ip6.c:127-161), the four UDP fields and mk_eth_hdr
 * (eth.h:89-109), for a batch of frames whose payload is already in place.
 * Everything is a function of a small per-socket tuple, a few per-iov values
 * and the payload bytes; no header byte is written on the host.  Plain C types,
 * little-endian layouts; "as stored" means network-order bytes, like the
 * record ports. */
#define WC_TX_BUILD_MAX_SOCKS 256
#define WC_TX_SOCK_CONNECTED 1u   /* w_connected(s): raddr / rport / dmac are the socket's   */
#define WC_TX_SOCK_ECN       2u   /* s->opt.enable_ecn                                        */

struct wc_tx_sock {               /* 52 bytes: what udp_tx reads of one w_sock and its engine */
    uint8_t  af;                  /* 4 or 6                                                   */
    uint8_t  flags;               /* WC_TX_SOCK_*                                             */
    uint16_t lport, rport;        /* as stored; rport ignored unless connected                */
    uint8_t  smac[6], dmac[6];    /* v->w->mac; s->dmac (ignored unless connected)            */
    uint8_t  pad[2];              /* ignored                                                  */
    uint8_t  laddr[16], raddr[16];/* af 4: bytes 0..3 count. laddr: s->ws_laddr, or for an    */
};                                /* unconnected socket the engine's interface address        */

struct wc_tx_dst {                /* 24 bytes: an unconnected send's v->wv_addr / wv_port and  */
    uint8_t  addr[16];            /* the MAC who_has() answered for it (eth.h:95-104)          */
    uint8_t  dmac[6];
    uint16_t port;                /* as stored */
};

struct wc_tx_desc {               /* 8 bytes per frame */
    uint16_t data_len;            /* v->len: UDP payload bytes                                */
    uint16_t ip_id;               /* ip->id as stored (the reference draws it at random and    */
                                  /* does not swap it, ip4.c:167-168); ignored for af 6        */
    uint8_t  sock;                /* index into the socket array                              */
    uint8_t  tos;                 /* v->flags                                                 */
    uint16_t dst;                 /* index into the destination array; ignored if connected   */
};

/* Pure host arithmetic (no GPU, no library state): WC_EINVAL for ns >
 * WC_TX_BUILD_MAX_SOCKS, a NULL array with ns > 0, an af other than 4 / 6 or
 * unknown flag bits; else WC_OK. */
int wc_tx_socks_check(const struct wc_tx_sock *socks, uint32_t ns);

/* Frame i starts at d_base + d_off[i] and may use slot_bytes bytes from there;
 * its payload already lies at + 14 + hl + 8 (hl = 20 for af 4, 40 for af 6:
 * where w_alloc_iov leaves v->buf).  The call writes the 14 + hl + 8 bytes in
 * front of the payload -- all of them, whatever they held -- and nothing else,
 * and sets d_frame_len[i] = 14 + hl + 8 + data_len (s->len, eth.c:124), 0 for
 * every status but the two sealed ones.
 *   Ethernet: dst = the socket's dmac if connected, else d_dsts[dst].dmac;
 *     src = smac; type 08 00 / 86 dd.
 *   IPv4 (ip4.c:153-189): 45, tos (| 2, ECT0, when (tos & 3) == 0 and the
 *     socket has WC_TX_SOCK_ECN), total length 28 + data_len, ip_id as stored,
 *     40 00 (DF), ttl ff, protocol 17, ip_cksum of these 20 bytes, src =
 *     laddr[0..3], dst = raddr[0..3] if connected, else d_dsts[dst].addr[0..3].
 *   IPv6 (ip6.c:127-161): the first word as the reference's ORs leave it on a
 *     zeroed word -- with tos & 3 set, byte 0 = 0x60 | tos >> 4 and byte 1 =
 *     (tos & 0x0f) << 4; without, byte 0 = 0x60 and byte 1 = 0 (the traffic
 *     class is dropped, ip6.c:133), and byte 2 = 0x20 if the socket has
 *     WC_TX_SOCK_ECN (ECN_ECT0 << 20 on the native word, ip6.c:138), else 0;
 *     byte 3 = 0 -- then payload length 8 + data_len, next header 17, hop
 *     limit ff, the 16-byte src and dst chosen as for IPv4.
 *     One deliberate difference from the reference: mk_ip6_hdr ORs into bytes
 *     1..3 of that word as the buffer left them; the build writes the whole
 *     word.
 *   UDP (udp.c:206-213): sport = lport, dport = rport if connected, else
 *     d_dsts[dst].port, len 8 + data_len, cksum = payload_cksum(ip, hl + 8 +
 *     data_len) with the field taken as 0, stored raw (a computed 0 stays 0,
 *     as in the seal); with WC_TX_ZERO_UDP_CKSUM in `flags` the field is
 *     written 0 and no payload byte is read (the per-socket option of
 *     udp.c:212 is a per-call flag, as for the seal: the caller batches by it).
 * d_status[i] is an enum wc_tx_status code; the checks run in this order and
 * the first that fails names it:
 *   1. sock >= ns, or the entry's af not 4 / 6:        WC_TX_MALFORMED
 *   2. unconnected socket and dst >= ndst:              WC_TX_MALFORMED
 *   3. 14 + hl + 8 + data_len > 65535:                  WC_TX_MALFORMED
 *   4. the frame is longer than slot_bytes:             WC_TX_TRUNCATED
 *   5. else WC_TX_SEALED, or WC_TX_SEALED_ZERO_UDP under the flag.
 * An error frame is untouched.  For no status is a byte outside [frame, frame
 * + frame_len) read or written, and no payload byte is ever written.
 * d_out_ip_hdr / d_out_udp (optional) receive the two values, 0 where none is
 * computed; *d_errors (device uint64, optional, accumulated) counts the
 * WC_TX_IS_ERROR frames.  flags: WC_TX_ZERO_UDP_CKSUM | WC_TX_NO_STORE (the
 * frames are only read, both out arrays required); any other bit is WC_EINVAL.
 * n = 0 is WC_OK and looks at no pointer.  WC_EINVAL, before a device is
 * touched: a NULL d_base / d_off / d_desc / d_frame_len / d_status, NULL
 * d_socks with ns > 0 or d_dsts with ndst > 0, ns > 256, ndst > 65536, d_desc
 * not 8-byte or d_socks / d_dsts not 4-byte aligned.  The frames of one call
 * must not overlap (they may share 16-byte chunks and cache lines).  One
 * asynchronous launch on `stream`; no library lock; the only atomic is the
 * error count's, one per wave. */
int wc_tx_build_ragged(void *d_base, const uint64_t *d_off, const struct wc_tx_desc *d_desc, uint64_t n,
                       const struct wc_tx_sock *d_socks, uint32_t ns,
                       const struct wc_tx_dst *d_dsts, uint32_t ndst, uint32_t slot_bytes, uint32_t flags,
                       uint16_t *d_frame_len, uint8_t *d_status,
                       uint16_t *d_out_ip_hdr, uint16_t *d_out_udp, uint64_t *d_errors, void *stream);

/* Host-memory frames and tables: the calling thread runs the same checks and
 * writes the headers of the frames that pass with both checksum fields 0 --
 * every such frame must lie inside [h_base, h_base + h_bytes), else WC_EINVAL
 * before any byte is written --, the device computes both values over the
 * host paths of wc_tx_seal_host (never the resident server; it never writes
 * host packet memory), and the calling thread stores them.  Synchronous;
 * *h_errors (optional) = the WC_TX_IS_ERROR count.  WC_TX_NO_STORE is
 * WC_EINVAL here. */
int wc_tx_build_host(void *h_base, uint64_t h_bytes, const uint64_t *h_off, const struct wc_tx_desc *h_desc,
                     uint64_t n, const struct wc_tx_sock *h_socks, uint32_t ns,
                     const struct wc_tx_dst *h_dsts, uint32_t ndst, uint32_t slot_bytes, uint32_t flags,
                     uint16_t *h_frame_len, uint8_t *h_status, uint64_t *h_errors);

/* --- RX replies: ICMP verdicts, echo and unreachable frames --------------- */

/* What the reference's RX path does with a frame beyond delivering it: the
 * MAC filter of eth_rx (eth.c:65-73), the address filter of ip4_rx / ip6_rx
 * (is_my_ip4 / is_my_ip6), the ICMP / ICMPv6 checksum verdict (icmp4.c:153-160,
 * icmp6.c:259-267), the echo replies (icmp4_tx / icmp6_tx) and the protocol
 * and port unreachables (ip4.c:133-137, udp.c:147-155).  All of it is a
 * function of the frame bytes and the engine table below; what changes engine
 * state (ARP, neighbour discovery) is handed to the host as WC_RR_HOST. */
#define WC_RX_MAX_IFADDR 16
struct wc_rx_ifaddr {     /* 52 bytes: one w_ifaddr (warpcore.h), as is_my_ip4 / is_my_ip6 read it */
    uint8_t af;           /* 4 or 6 */
    uint8_t pad[3];       /* ignored */
    uint8_t addr[16];     /* af 4: bytes 0..3 count, as in struct wc_rx_sock */
    uint8_t bcast[16];    /* af 4: bcast4 in bytes 0..3; af 6: bcast6 */
    uint8_t snma[16];     /* af 6: snma6; ignored for af 4 */
};
struct wc_rx_engine {     /* 844 bytes, little-endian, what the RX path reads of a w_engine */
    uint8_t  mac[6];      /* w->mac */
    uint16_t mtu;         /* w->mtu */
    uint32_t naddr;       /* <= WC_RX_MAX_IFADDR */
    struct wc_rx_ifaddr addr[WC_RX_MAX_IFADDR];
};

/* Pure host arithmetic (no GPU, no library state), like wc_tx_socks_check:
 * WC_EINVAL for a NULL pointer, naddr > 16, an af other than 4 / 6 among the
 * first naddr entries, an af-6 entry after an af-4 entry (backend_addr_config
 * lays them out IPv6 first, ifaddr.c:94-146, and the reply sources depend on
 * it), or mtu < 68 -- the reference has no such rule, but its w->mtu -
 * sizeof(*src_ip) (icmp6.c:164) wraps below 40; else WC_OK.  The reply sources
 * are the first af-4 entry for IPv4 (ifaddr[addr4_pos], ip4.c:180) and entry
 * 0 for IPv6 (ip6.c:155). */
int wc_rx_engine_check(const struct wc_rx_engine *e);

enum wc_rx_reply_action {        /* uint8, all < 32 so wc_rx_select masks apply */
    WC_RR_NONE = 0,              /* nothing to send, nothing for the host */
    WC_RR_HOST = 1,              /* the host's: changes engine state (ARP; ICMPv6 NSOL / NADV, checksum verified) */
    WC_RR_FILTERED = 2,          /* MAC or IP destination is not ours (eth.c:65-73, ip4.c:103-108, ip6.c:98-103) */
    WC_RR_ICMP_BAD_CKSUM = 3,    /* icmp4.c:156, icmp6.c:263: dropped */
    WC_RR_MALFORMED = 4,         /* a length the reference would wrap, or a byte it would read past the frame: no reply */
    WC_RR_NO_ROOM = 5,           /* the reply is longer than slot_bytes: no reply */
    WC_RR_ECHO4 = 8, WC_RR_ECHO6 = 9,
    WC_RR_UNREACH_PORT4 = 10, WC_RR_UNREACH_PORT6 = 11, WC_RR_UNREACH_PROTO4 = 12,
};
#define WC_RR_MASK_REPLY (0x1F00u)

/* Behind a wc_rx_verdict_ragged / wc_rx_deliver_ragged (and optionally a
 * wc_rx_demux) of the same frames on the same stream: it reads their
 * d_verdict and d_sock (optional) and does not decide again what they decided.
 * d_action[i] = frame i's enum wc_rx_reply_action code, d_reply_len[i] = the
 * reply's frame length for a reply action, else 0.  d_eng: the table in device
 * memory.  With d_list / d_count (both or neither: checked first, for every
 * n): wc_rx_select(d_action, n, WC_RR_MASK_REPLY, ...) on the same stream,
 * with d_scratch of wc_rx_select_scratch(n) bytes.
 *
 * The chain, in the reference's order; the first hit names the code.  "ip" is
 * the frame from byte 14, hl = 4 * IHL as the byte gives it (values below 20
 * included, as the reference would use them) or 40, flen the frame length;
 * lengths are computed in 32 bits unless a wrap is named.
 *   1. The verdict is a drop (WC_RX_IS_DROP) or above 9:            NONE.
 *   2. Frame bytes 0..5 differ from mac and from ff x 6, and bytes 0..1 are
 *      not 33 33 (eth.c:65-67):                                     FILTERED.
 *   3. Verdict NOT_IP:                                              HOST.
 *   4. IPv4: for no af-4 entry is dst equal to addr, bcast or 255.255.255.255
 *      (is_my_ip4 with match_bcast; with no af-4 entry nothing matches);
 *      IPv6: for no af-6 entry is dst equal to addr, snma or bcast:  FILTERED.
 *      One deliberate difference: the reference's IPv6 loop (ip6.c:173-187)
 *      also compares against the 16 union bytes of IPv4 entries; the plan
 *      compares af-6 entries only.
 *   5. Verdict OK / OK_NO_CKSUM: NONE unless d_sock is given and d_sock[i] ==
 *      WC_RX_SOCK_UNBOUND and the frame's SOURCE address is an addr of its
 *      family in the table (no broadcast match) -- udp.c:150-153 as it stands;
 *      then UNREACH_PORT4 with reply length 50 + hl, or UNREACH_PORT6 with
 *      reply length 110 (its ICMP data is 48 bytes from frame byte 54 on:
 *      ip6_data(buf), icmp6.c:163, 210); flen < 102 is MALFORMED.
 *   6. Verdict NOT_UDP, IPv4, protocol != 1: UNREACH_PROTO4, reply length 50 +
 *      hl; it copies hl + 8 bytes from ip, flen < 14 + hl + 8 is MALFORMED.
 *   7. Verdict NOT_UDP, IPv4, protocol 1: icmp_len = MIN((ip_len - hl) &
 *      0xFFFF, flen - 14 - hl); ip_cksum(ip + hl, icmp_len) != 0 (a zero
 *      length sums to 0xFFFF) is ICMP_BAD_CKSUM; a type other than 8 is NONE;
 *      for type 8, with t = MIN(ip_len, mtu): t < hl + 8 is MALFORMED (the
 *      uint16 wrap of icmp4.c:91), 14 + t > flen is MALFORMED (the reference
 *      copies its neighbour's bytes), else ECHO4 with data_len = t - hl - 8
 *      and reply length 42 + data_len.
 *   8. Verdict NOT_UDP, IPv6, next header != 58:                    NONE.
 *   9. Verdict NOT_UDP, IPv6, next header 58: icmp_len = MIN(ip6_len, flen -
 *      54); payload_cksum(ip, icmp_len + 40) != 0 is ICMP_BAD_CKSUM; flen < 55
 *      (no type byte) is MALFORMED; types 135 / 136 are HOST; for type 128,
 *      with t = MIN(ip6_len, mtu - 40): t < 8 is MALFORMED (icmp6.c:202), 54 +
 *      t > flen is MALFORMED, else ECHO6 with data_len = t - 8 and reply
 *      length 62 + data_len; any other type is NONE.
 *  10. A reply longer than slot_bytes:                              NO_ROOM.
 * n = 0 is WC_OK, writes *d_count = 0 where given and looks at no other
 * pointer.  WC_EINVAL: n > 2^32, slot_bytes > 65535, a NULL d_base / d_off /
 * d_frame_len / d_verdict / d_eng / d_action / d_reply_len, d_eng not 4-byte
 * aligned, a list without a 4-byte-aligned d_scratch.  Asynchronous on
 * `stream`: one launch, four with the list; no library lock, no atomic, no
 * wait between workgroups, and the same input gives the same output.  No byte
 * outside a frame is read (reads are the aligned 16-byte chunks that overlap
 * it). */
int wc_rx_reply_plan(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                     const uint8_t *d_verdict, const uint8_t *d_sock /* optional */,
                     const struct wc_rx_engine *d_eng, uint32_t slot_bytes,
                     uint8_t *d_action, uint16_t *d_reply_len,
                     uint32_t *d_list, uint64_t *d_count, void *d_scratch, void *stream);

/* Reply j, for j < MIN(*d_count, m), answers frame d_list[j]: it is written
 * at d_out_base + d_out_off[j], may use slot_bytes bytes there, and
 * d_out_len[j] is its length.  For every other j < m d_out_len[j] = 0 and the
 * slot is untouched (the reference's "no more bufs; ICMP not sent").
 * *d_built is written, not accumulated: the number of j with a non-zero
 * length.  *d_count is read on the device: one launch, no host
 * synchronisation.  The build derives every length and bound again from the
 * frame -- the MALFORMED / NO_ROOM conditions above, that the header bytes a
 * reply reads lie inside the frame (flen >= 34 / 54), a list index >= n, an
 * action that is no reply action -- and writes length 0 and touches nothing
 * where they fail, so a stale action byte cannot make it read or write out of
 * range.  It does not verify checksums or filters again.  RX frames and reply
 * slots must not overlap, nor reply slots each other (they may share 16-byte
 * chunks and cache lines, as in the TX build); no byte outside [slot, slot +
 * reply length) is written, none outside the source frame read (reads are
 * aligned dwords inside the 16-byte chunks that overlap it).
 *   Ethernet: dst = the request's bytes 6..11, src = mac, type 08 00 / 86 dd.
 *   IPv4 (mk_ip4_hdr(v, 0), v->flags = 0): 45 00, total length reply length -
 *     14, d_ip_id[j] as stored (00 00 when d_ip_id is NULL; the reference
 *     draws it at random, ip4.c:167-168), 40 00, ff, 01, ip_cksum of the 20
 *     bytes, src = the first af-4 address, dst = the request's IP source.
 *   ICMP: ECHO4 00 00, checksum, the request's ICMP bytes 4..7, then request
 *     bytes [14 + hl + 8, 14 + t); UNREACH_PORT4 03 03, checksum, four zero
 *     bytes, then request bytes [14, 14 + hl + 8); UNREACH_PROTO4 03 02, then
 *     the same.  Checksum: ip_cksum(icmp, 8 + data_len) with the field taken
 *     as 0, stored raw.
 *   IPv6 (mk_ip6_hdr(v, 0)): first word 60 00 00 00, written whole (the same
 *     deliberate difference from the reference's OR as in the TX build),
 *     payload length reply length - 54, 3a, ff, src = entry 0's address, dst
 *     = the request's source.
 *   ICMPv6: ECHO6 81 00, checksum, the request's bytes 58..61, then request
 *     bytes [62, 54 + t); UNREACH_PORT6 01 04, checksum, four zero bytes, then
 *     request bytes [54, 102).  Checksum: payload_cksum(ip, reply length - 14)
 *     with the field taken as 0, stored raw.
 * m = 0 is WC_OK, writes *d_built = 0 and looks at no other pointer; n = 0
 * writes that and m zero lengths.  WC_EINVAL: n > 2^32, slot_bytes > 65535, a
 * NULL d_built, a NULL d_out_len with m > 0; with m > 0 and n > 0 any other
 * NULL pointer but d_ip_id, or d_eng not 4-byte aligned.  The only atomic is
 * the built count's, one per workgroup of a grid no larger than the device
 * holds at once. */
int wc_rx_reply_build(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                      const uint8_t *d_action, const uint32_t *d_list, const uint64_t *d_count,
                      const struct wc_rx_engine *d_eng,
                      void *d_out_base, const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                      const uint16_t *d_ip_id /* optional, m entries */,
                      uint16_t *d_out_len, uint64_t *d_built, void *stream);

/* --- RX neighbours: ARP / ND replies and cache updates --------------------- */

/* What the reference does with the frames wc_rx_reply_plan marks WC_RR_HOST:
 * arp_rx (arp.c:157-198) with its is-at reply (arp_is_at, arp.c:65-100), and
 * the neighbour solicitation / advertisement branches of icmp6_rx
 * (icmp6.c:270-322) with the advertisement icmp6_tx writes (icmp6.c:168-193,
 * 221-228).  All of it is a function of the frame bytes and the engine table;
 * the host applies the (address, MAC) records to its cache in order
 * (neighbor_update) and posts the built frames -- or hands the records to
 * wc_neigh_apply ("TX neighbours" below), which keeps the cache, the who_has
 * lookup and its solicitations on the device. */
enum wc_rx_neigh_action {        /* uint8, all < 32 so wc_rx_select masks apply */
    WC_RN_NONE = 0,              /* nothing to do */
    WC_RN_MALFORMED = 4,         /* a byte the reference would read lies past the frame */
    WC_RN_UPDATE4 = 8,           /* ARP: cache update only */
    WC_RN_ARP_IS_AT = 9,         /* ARP request for us: update plus a 42-byte is-at */
    WC_RN_NADV = 10,             /* solicitation for us: update plus an 86-byte advertisement */
    WC_RN_UPDATE6 = 11,          /* advertisement received: update only */
};
#define WC_RN_MASK_REPLY  (0x600u)
#define WC_RN_MASK_UPDATE (0xF00u)

struct wc_neigh_update {         /* 24 bytes: what neighbor_update receives */
    uint8_t af;                  /* 4 or 6; 0: an empty record */
    uint8_t action;              /* the enum wc_rx_neigh_action code it came from */
    uint8_t mac[6];
    uint8_t addr[16];            /* af 4: bytes 0..3, the rest 0 */
};

/* Behind a wc_rx_reply_plan of the same frames on the same stream: it reads
 * its d_action and does not decide again what the calls in front decided (the
 * MAC filter, the IPv6 address filter, the ICMPv6 checksum).  d_nact[i] = frame
 * i's enum wc_rx_neigh_action code.  With d_rlist / d_rcount:
 * wc_rx_select(d_nact, n, WC_RN_MASK_REPLY, ...); with d_ulist / d_ucount: the
 * same with WC_RN_MASK_UPDATE; both on the same stream, one after the other
 * through the one d_scratch of wc_rx_select_scratch(n) bytes.  For each pair
 * both pointers are given or neither: checked first, for every n.
 *
 * The chain; the first hit names the code.  Frame bytes are numbered from the
 * Ethernet header, flen is the frame length.
 *   1. d_action[i] != WC_RR_HOST (or flen < 14: no EtherType):      NONE.
 *   2. Bytes 12..13 are 08 06 (eth.c:80-83):
 *      a. no af-4 entry in the table (w->have_ip4):                  NONE.
 *      b. flen < 42:                                                 MALFORMED.
 *      c. bytes 14..15 are not 00 01, or byte 18 is not 6 (arp.c:161): NONE.
 *      d. bytes 16..17 are not 08 00, or byte 19 is not 4 (arp.c:167): NONE.
 *      e. bytes 20..21: 00 01 -- ARP_IS_AT if bytes 38..41 equal the addr of
 *         an af-4 entry (is_my_ip4 without the broadcast match: bcast and
 *         255.255.255.255 do not match), else UPDATE4 (the reference updates
 *         the cache for requests that are not for us too, arp.c:181-183, 196);
 *         00 02 -- UPDATE4; anything else -- NONE.
 *   3. Bytes 12..13 are 86 dd:
 *      a. flen < 55, or byte 20 is not 58, or byte 54 is neither 135 nor 136
 *         (a stale action byte):                                     NONE.
 *      b. flen < 78 (the 16 target bytes 62..77):                    MALFORMED.
 *      c. byte 54 is 136:                                            UPDATE6.
 *      d. byte 54 is 135: NADV if bytes 62..77 equal the addr of an af-6
 *         entry (is_my_ip6 without snma / bcast; af-6 entries only, the reply
 *         plan's deliberate difference), else NONE (icmp6.c:312-321: no
 *         update either).
 *   4. Any other EtherType:                                          NONE.
 * n = 0 is WC_OK and writes 0 to whichever counts are given.  WC_EINVAL: a
 * list without its count or a count without its list, n > 2^32, a NULL d_base
 * / d_off / d_frame_len / d_action / d_eng / d_nact, d_eng not 4-byte aligned,
 * a list without a 4-byte-aligned d_scratch.  Asynchronous on `stream`: one
 * launch and three per list; no library lock, no atomic, and the same input
 * gives the same output.  No byte outside a frame is read (reads are the
 * aligned 16-byte chunks that overlap it), and no frame byte at all of a frame
 * whose action is not WC_RR_HOST. */
int wc_rx_neigh_plan(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                     const uint8_t *d_action, const struct wc_rx_engine *d_eng, uint8_t *d_nact,
                     uint32_t *d_rlist, uint64_t *d_rcount, uint32_t *d_ulist, uint64_t *d_ucount,
                     void *d_scratch, void *stream);

/* For j < MIN(*d_count, m), d_upd[j] is the record of frame d_list[j] (the
 * plan's d_ulist / d_ucount; *d_count is read on the device).  The records
 * come out in ring order, so applying them in order leaves the cache as the
 * reference would.
 *   UPDATE4, ARP_IS_AT: af 4, addr = bytes 28..31 (spa), mac = bytes 22..27 (sha).
 *   UPDATE6: af 6, addr = bytes 62..77 (the target); NADV: af 6, addr = the IPv6
 *     source, bytes 22..37 (icmp6.c:316-318).  mac, for both (icmp6.c:272-282,
 *     295-304): with data_len = MIN(ip6 payload length, flen - 62), bytes
 *     80..85 if data_len >= 24 and bytes 78..79 are 01 01, else bytes 6..11 (the
 *     reference tests option type 1 on a received advertisement too).
 * The record is all zero where the index is >= n, the code is no update code
 * or the frame is shorter than 42 / 78, and for MIN(*d_count, m) <= j < m.
 * m = 0 is WC_OK and looks at no pointer; n = 0 writes m zero records.
 * WC_EINVAL: n > 2^32, with m > 0 a NULL or not 4-byte-aligned d_upd, with m >
 * 0 and n > 0 any other NULL pointer.  One launch, no atomic; no byte outside a
 * frame is read (reads are aligned dwords that overlap it). */
int wc_rx_neigh_updates(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                        const uint8_t *d_nact, const uint32_t *d_list, const uint64_t *d_count,
                        uint32_t m, struct wc_neigh_update *d_upd, void *stream);

/* The contract of wc_rx_reply_build for the plan's d_rlist / d_rcount: reply
 * j < MIN(*d_count, m) answers frame d_list[j], is written at d_out_base +
 * d_out_off[j] and d_out_len[j] is its length; *d_built is written, not
 * accumulated.  d_out_len[j] is 0 and the slot untouched where the index is >=
 * n, the code is no reply code, the frame is shorter than 42 / 78, slot_bytes
 * is below 42 / 86, or j is at or past the count.  Nothing outside [slot, slot
 * + length) is written; all stores are plain vector stores.
 *   ARP_IS_AT, 42 bytes (arp.c:78-96): dst = request bytes 22..27 (its sha, not
 *     its Ethernet source), src = mac, 08 06; 00 01 08 00 06 04 00 02; sha =
 *     mac, spa = request bytes 38..41, tha = request bytes 22..27, tpa =
 *     request bytes 28..31.
 *   NADV, 86 bytes: dst = request bytes 6..11, src = mac, 86 dd; 60 00 00 00
 *     (written whole, as the existing replies), 00 20, 3a, ff, src = entry 0's
 *     address, dst = request bytes 22..37; 88 00, checksum, 60 00 00 00,
 *     request bytes 62..77, 02 01, mac.  Checksum: payload_cksum(ip, 72) with
 *     the field taken as 0, stored raw.  A reference quirk is kept: icmp6_tx's
 *     source-link-address test reads the ICMPv6 type and code bytes
 *     (icmp6.c:163, 173-175), never 01 01 for a solicitation, so the Ethernet
 *     destination is always the request's source MAC.
 * m = 0 is WC_OK, writes *d_built = 0 and looks at no other pointer; n = 0
 * writes that and m zero lengths.  WC_EINVAL: as wc_rx_reply_build.  The only
 * atomic is the built count's, one per workgroup of a grid no larger than the
 * device holds at once. */
int wc_rx_neigh_build(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                      const uint8_t *d_nact, const uint32_t *d_list, const uint64_t *d_count,
                      const struct wc_rx_engine *d_eng,
                      void *d_out_base, const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                      uint16_t *d_out_len, uint64_t *d_built, void *stream);

/* --- RX drain: the whole per-ring RX plan in one call ---------------------- */

/* What one poll of a netmap ring delivers is 256 to 4096 frames, and at that
 * size the chain wc_rx_deliver_ragged -> wc_rx_demux -> wc_rx_reply_plan ->
 * wc_rx_neigh_plan costs its seventeen launches and nothing else.  wc_rx_drain
 * is that chain as one call: for n <= WC_RX_DRAIN_SMALL it is TWO launches
 * (one wave per 64 frames for the six per-frame arrays, then one workgroup for
 * the five lists and their counts); for a larger n it issues the four calls
 * itself, so a caller has one entry point for any ring.  The build calls
 * (wc_rx_reply_build, wc_rx_neigh_updates, wc_rx_neigh_build) and
 * wc_neigh_apply follow it unchanged and consume its lists and counts.
 *
 * The contract: for every n, every output array holds exactly the bytes
 *   wc_rx_deliver_ragged(d_base, d_off, d_frame_len, n, verdict, rec, NULL, NULL, drops, NULL, st);
 *   wc_rx_demux(d_base, d_off, rec, n, d_tab, ns, sock, list, start, d_scratch, st);
 *   wc_rx_reply_plan(d_base, d_off, d_frame_len, n, verdict, sock, d_eng, slot_bytes,
 *                    action, reply_len, rlist, rcount, d_scratch, st);
 *   wc_rx_neigh_plan(d_base, d_off, d_frame_len, n, action, d_eng,
 *                    nact, nrlist, nrcount, ulist, ucount, d_scratch, st);
 * leave there: list entries at and past a count keep what they held, all 256
 * start entries are written, *drops is accumulated and the four counts (start
 * [255], *rcount, *nrcount, *ucount) are written; no byte outside a frame is
 * read, the RX buffer is not written, and the same input gives the same
 * output.  Every member of *out is a device pointer with the alignment and
 * size its call above asks for (rec: 16-byte aligned; the lists: n entries),
 * and every member but drops is required.
 *
 * d_scratch: wc_rx_drain_scratch(n) bytes of device memory, 4-byte aligned,
 * the caller's, one per call in flight -- enough for the calls above, which run
 * one after another on the stream and share it.  The function is pure
 * arithmetic, 0 for n = 0 and never decreasing in n.
 *
 * n = 0 is WC_OK: it writes the four zero counts and an all-zero start, and
 * looks at no other pointer (d_base, d_tab, d_eng, d_scratch and the other
 * members of *out may be NULL).  WC_EINVAL: a NULL out, n > 2^32, ns > 254, a
 * NULL start / rcount / nrcount / ucount; and with n > 0: slot_bytes > 65535, a
 * NULL d_base / d_off / d_frame_len / d_tab / d_eng or other required member,
 * d_tab or d_eng not 4-byte aligned, rec not 16-byte aligned, a d_scratch that
 * is NULL or not 4-byte aligned.  Asynchronous on `stream`, no library lock.
 * The two launches: no workgroup waits for another, the only atomic is the drop
 * count's (one per wave with a drop), all stores are plain vector stores. */
#define WC_RX_DRAIN_SMALL 4096u

struct wc_rx_drain_out {          /* device pointers; all required except drops */
    uint8_t *verdict;  struct wc_rx_record *rec;  uint64_t *drops;  /* as wc_rx_deliver_ragged; drops accumulated, optional */
    uint8_t *sock;     uint32_t *list;  uint64_t *start;            /* as wc_rx_demux: 256 start entries */
    uint8_t *action;   uint16_t *reply_len;  uint32_t *rlist;  uint64_t *rcount;   /* as wc_rx_reply_plan, d_sock given */
    uint8_t *nact;     uint32_t *nrlist; uint64_t *nrcount; uint32_t *ulist; uint64_t *ucount; /* as wc_rx_neigh_plan */
};
uint64_t wc_rx_drain_scratch(uint64_t n);
int wc_rx_drain(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                const void *d_tab, uint32_t ns, const struct wc_rx_engine *d_eng, uint32_t slot_bytes,
                const struct wc_rx_drain_out *out /* host struct */, void *d_scratch, void *stream);

/* --- RX answer: the builds behind the drain and the apply in one call ------ */

/* Behind every drain the caller ran wc_rx_reply_build, wc_rx_neigh_updates,
 * wc_rx_neigh_build and wc_neigh_apply ("TX neighbours" below): five launches
 * and two memsets for the handful of frames of a ring that want an answer or
 * carry a neighbour update.  wc_rx_answer is that chain as one call: with r_m,
 * n_m and u_m all <= WC_RX_ANSWER_SMALL (and, where tab is given, u_m <=
 * WC_RX_ANSWER_SMALL_APPLY) it is TWO launches and no memset (one
 * grid whose workgroups are split between the three builds, then one workgroup
 * for the two built counts and the apply); above any of them it issues the
 * four calls itself, so a caller has one entry point for any size.  A ring turn
 * on the device is wc_rx_drain -> wc_rx_answer -> wc_tx_pump, two launches each,
 * with no host read in between.
 *
 * The contract: for every n and every r_m / n_m / u_m, every output holds
 * exactly what this chain leaves there, run on the same stream:
 *   wc_rx_reply_build  (d_base, d_off, d_frame_len, n, action, rlist,  rcount,  d_eng, r_out_base, r_out_off, r_m, slot_bytes, ip_id, r_out_len, r_built, st);
 *   wc_rx_neigh_updates(d_base, d_off, d_frame_len, n, nact,   ulist,  ucount,  u_m, upd, st);
 *   wc_rx_neigh_build  (d_base, d_off, d_frame_len, n, nact,   nrlist, nrcount, d_eng, n_out_base, n_out_off, n_m, slot_bytes, n_out_len, n_built, st);
 *   if (tab) wc_neigh_apply(tab, upd, ucount, u_m, dropped, d_scratch, st);
 * byte for byte: the slots, with nothing outside [slot, slot + length) written;
 * both length arrays over all m entries; both built counts, written and not
 * accumulated; all u_m records, the zero ones included.  For the table the
 * contract is wc_neigh_apply's own, not byte for byte: read through lookups it
 * is the chain's; which new keys a full table keeps stays unspecified; which
 * entry a key lands in may differ; *dropped is accumulated by the same number.
 * The RX buffer is not written, no byte outside a frame is read, and the same
 * input gives the same output.  Every rule of the four calls holds for its
 * part: m = 0 looks at no pointer of that part, except that both built counts
 * are always written; n = 0 gives zero lengths and zero records; a stale action
 * byte or a list index >= n gives length 0 and an untouched slot.
 * One precondition the chain does not have: the reply slots and the neighbour
 * slots must not overlap each other -- they now belong to one launch, where the
 * chain would simply have overwritten.
 *
 * d_scratch: wc_rx_answer_scratch(u_m) = wc_neigh_apply_scratch(u_m) bytes of
 * device memory, 4-byte aligned, the caller's, one per call in flight; required
 * only when tab != NULL and u_m > 0.  Pure arithmetic, 0 at 0 and never
 * decreasing (the two launches use none, but ask for the same).
 *
 * WC_EINVAL, before a device is touched: a NULL io, r_built or n_built; n >
 * 2^32; slot_bytes > 65535; for each part with m > 0 (and n > 0 where its call
 * says so) the NULL and alignment rules of its call; with tab and u_m > 0,
 * wc_neigh_apply's rules for tab, upd, ucount and d_scratch.  Asynchronous on
 * `stream`, no library lock.  The two launches: no workgroup waits for another,
 * nothing spins, all stores are plain vector stores or the table's own atomics
 * (and one atomic add on *dropped). */
#define WC_RX_ANSWER_SMALL 4096u        /* entries per list: r_m, n_m and u_m */
#define WC_RX_ANSWER_SMALL_APPLY 1024u  /* u_m where tab is given: one workgroup's claim and
                                         * commit of more records measured slower than the chain */

struct wc_rx_answer_io {                /* host struct; device pointers */
    /* in: what wc_rx_drain (or the two plans) left */
    const uint8_t *action;  const uint32_t *rlist;  const uint64_t *rcount;
    const uint8_t *nact;    const uint32_t *nrlist; const uint64_t *nrcount;
    const uint32_t *ulist;  const uint64_t *ucount;
    /* replies, as wc_rx_reply_build */
    void *r_out_base; const uint64_t *r_out_off; uint32_t r_m;
    const uint16_t *ip_id /* optional */; uint16_t *r_out_len; uint64_t *r_built;
    /* ARP is-at / neighbour advertisements, as wc_rx_neigh_build */
    void *n_out_base; const uint64_t *n_out_off; uint32_t n_m;
    uint16_t *n_out_len; uint64_t *n_built;
    /* update records, as wc_rx_neigh_updates */
    uint32_t u_m; struct wc_neigh_update *upd;
    /* the device neighbour cache, as wc_neigh_apply; tab NULL: no apply */
    void *tab; uint64_t *dropped /* optional, accumulated */;
};
uint64_t wc_rx_answer_scratch(uint32_t u_m);
int wc_rx_answer(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
                 const struct wc_rx_engine *d_eng, uint32_t slot_bytes,
                 const struct wc_rx_answer_io *io /* host struct */, void *d_scratch, void *stream);

/* --- RX echo: delivered datagrams become a TX batch on the device ---------- */

/* The reference's own server application (bin/inetd.c:161-169): port 7 hands
 * every received iov back to w_tx -- sq_concat(&o, &i); w_tx(s, &o) -- with the
 * address, port and TOS udp_rx left in it (udp.c:107-110, 141), and udp_tx
 * writes the headers in front of v->buf; port 9 discards.  The drain ends with
 * each socket's delivered frames as a run of list / start and a wc_rx_record
 * per frame; the pump begins with a wc_tx_desc per frame, a wc_tx_dst / d_af
 * table and payloads behind their header space.  wc_rx_echo gets from the
 * first to the second in ONE launch for every n and m, so that the ping /
 * inetd pair is wc_rx_drain -> wc_rx_answer -> wc_rx_echo -> wc_tx_pump on one
 * stream with no host read.
 *
 * Inputs.  d_rec (n records), d_list (n entries) and d_start (256) are what
 * wc_rx_drain or wc_rx_demux left.  d_map has ns entries (ns <= 254): a value
 * <= 255 is the wc_tx_sock index RX socket s answers from, any value above 255
 * (WC_ECHO_OFF) means the socket is not echoed.  The unbound run (start[254 ..
 * 255]) is never echoed.
 *
 * Echo order.  Sockets ascending, each socket's run in ring order (inetd.c's
 * sl_foreach / w_rx / w_tx, one socket after another): entry j is the j-th
 * frame of the concatenated runs of the switched-on sockets.  A run is
 * [start[s], start[s+1]) and counts as empty unless start[s] <= start[s+1] <=
 * n, so stale starts are harmless.  E is the total; *count = E is written, not
 * accumulated.  Entries j >= m are dropped: the caller sees E > m.
 *
 * Entry j < min(E, m), from frame i = the list entry, gets status[j]; the
 * first rule that holds names it:
 *   WC_EC_STALE    i >= n, the record's af is not 4 / 6, or the record is none a
 *                  delivery writes for a frame of d_frame_len[i] bytes: hl
 *                  below hl_tx, data_off not 14 + hl + 8, or the source
 *                  address not inside the frame
 *   WC_EC_SHORT    data_off + data_len > frame_len (the record's documented
 *                  OK_NO_CKSUM case)
 *   WC_EC_NO_ROOM  copy mode and 14 + hl_tx + 8 + data_len > out_slot_bytes
 *   WC_EC_ECHO     otherwise; then, with hl_tx = 20 for af 4 and 40 for af 6:
 *     desc[j] = { data_len = rec.data_len, ip_id = d_ip_id ? d_ip_id[j] : 0,
 *                 sock = (uint8_t)d_map[s], tos = rec.tos, dst = j } -- udp_tx
 *       reading v->len / v->flags; the IP id stays the caller's random draw, as
 *       in wc_rx_reply_build.
 *     dsts[j] = { addr = the frame's IP source at rec.src_off (af 4: 4 bytes
 *       and 12 zero bytes; af 6: 16 bytes), port = rec.sport as stored, dmac =
 *       frame bytes 6..11 }.  af[j] = rec.af.
 *       Deliberate difference 1: dmac, the sender's Ethernet source, is a
 *       PLACEHOLDER.  The reference asks who_has for every send, and so does
 *       wc_tx_pump, whose resolve overwrites the six bytes of every entry; only
 *       a caller that hands the batch to wc_tx_build_ragged directly sends to
 *       the placeholder.
 *     Copy mode (d_out_base and d_out_off given, out->tx_off NULL): the
 *       data_len payload bytes are copied to d_out_base + d_out_off[j] + 14 +
 *       hl_tx + 8, where wc_tx_build_ragged expects them; nothing else of the
 *       slot is written.  No byte outside [frame, frame + frame_len) is USED;
 *       bytes are LOADED as the aligned 16-byte chunks and dwords that overlap
 *       the payload (here and for the address and MAC fields in both modes),
 *       so a load can take up to 15 bytes in front of the frame or behind its
 *       end -- never outside the aligned 16-byte chunks that overlap the frame.
 *       The RX buffer must therefore be readable up to the next 16-byte
 *       boundary behind its last frame, as for every RX call of this library
 *       (any device allocation is).
 *       The slots must not overlap each other or the RX buffer.
 *     In-place mode (d_out_base and d_out_off NULL, out->tx_off given): no
 *       payload byte is read or written; tx_off[j] = d_off[i] + (rec.hl -
 *       hl_tx), so that the pump, called with d_base and tx_off, writes its
 *       headers directly in front of the received payload -- the reference's
 *       zero-copy echo.
 *       Deliberate difference 2: for an IPv4 frame with options (hl > 20) the
 *       reference builds at v->base and would send the option bytes as
 *       payload; the echo shifts the frame start instead.  The built frame
 *       starts up to 40 bytes into the RX slot, so the caller passes the pump a
 *       slot_bytes reduced by the largest shift, 40.
 *   src[j] (optional) = i wherever i < n, else 0xFFFFFFFF.
 * Exactly one of the two modes must be selected (with m > 0).
 *
 * Inert entries -- every j in [min(E, m), m) (WC_EC_NONE, src 0xFFFFFFFF) and
 * every SHORT / NO_ROOM / STALE entry -- are written so that any later build
 * or pump refuses them without touching a slot: desc = { data_len 0xFFFF,
 * ip_id 0, sock 0, tos 0, dst = j } (the build's check 3: WC_TX_MALFORMED, the
 * frame untouched), dsts[j] all zero and af[j] = 0 (resolve: WC_NR_BAD_AF),
 * tx_off[j] = 0, nothing copied.  All m entries of every array are therefore
 * always written, as wc_rx_answer does for its records: the caller calls the
 * pump with n = ndst = m and never reads E.  The inert entries count in the
 * pump's *errors; status tells them apart.  *skipped (optional, accumulated)
 * grows by the SHORT + NO_ROOM + STALE entries below m.
 *
 * m = 0 is WC_OK: it writes *count and looks at no other output.  n = 0 or ns
 * = 0 gives E = 0 and m inert entries, and looks at no RX pointer (d_base,
 * d_off, d_frame_len, d_rec, d_list, d_start and d_map may be NULL).
 * WC_EINVAL, before a device is touched: a NULL out or count; n > 2^32, ns >
 * 254, m > WC_RX_ECHO_MAX or out_slot_bytes > 65535; with m > 0 a NULL desc /
 * dsts / af / status, both modes or neither; desc not 8-byte aligned, dsts not
 * 4-byte aligned, d_rec not 16-byte aligned, tx_off / d_out_off not 8-byte
 * aligned; with n > 0 and ns > 0 a NULL d_base / d_off / d_frame_len / d_rec /
 * d_list / d_start / d_map.  Asynchronous on `stream`, no library lock, no
 * scratch.  The one launch: no workgroup waits for another, nothing spins, the
 * only atomic is *skipped's (one per wave with a skipped entry), all global
 * stores are plain vector stores, and the same input gives the same output. */
enum wc_rx_echo_status {   /* uint8, all < 32 so wc_rx_select masks apply */
    WC_EC_ECHO    = 0,     /* descriptor, destination and payload are ready for the pump */
    WC_EC_NONE    = 4,     /* j at or past the echo count: padding */
    WC_EC_SHORT   = 8,     /* data_off + data_len > frame_len: nothing is read past the frame */
    WC_EC_NO_ROOM = 9,     /* copy mode: 14 + hl_tx + 8 + data_len > out_slot_bytes */
    WC_EC_STALE   = 10,    /* list index >= n, or a record no delivery wrote for the frame */
};
#define WC_ECHO_OFF 0xFFFFu        /* d_map[s]: socket s is not echoed (inetd's discard) */
#define WC_RX_ECHO_MAX 65536u      /* m: wc_tx_desc.dst is 16 bits, the build's ndst limit */

struct wc_rx_echo_out {            /* host struct of device pointers, m entries each */
    struct wc_tx_desc *desc; struct wc_tx_dst *dsts; uint8_t *af;
    uint8_t *status; uint32_t *src /* optional: the ring index i of entry j */;
    uint64_t *tx_off  /* in-place mode only */;
    uint64_t *count   /* written: E, the number of echo frames found */;
    uint64_t *skipped /* optional, accumulated: SHORT + NO_ROOM + STALE entries below m */;
};
int wc_rx_echo(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
               const struct wc_rx_record *d_rec, const uint32_t *d_list, const uint64_t *d_start,
               const uint16_t *d_map, uint32_t ns, const uint16_t *d_ip_id /* optional, m */,
               void *d_out_base, const uint64_t *d_out_off, uint32_t out_slot_bytes, uint32_t m,
               const struct wc_rx_echo_out *out /* host struct */, void *stream);

/* --- TX neighbours: device neighbour cache, batched who_has, solicitations - */

/* What lies between "RX produces update records" and "TX consumes destination
 * MACs" in the reference: the hash table of neighbor.c (neighbor_update,
 * neighbor.c:48-65; neighbor_find, 75-82), the who_has loop (95-118) and the two
 * frames it sends, arp_who_has (arp.c:107-142) and icmp6_nsol (icmp6.c:85-129).
 * A ring's ARP replies reach the next TX batch's Ethernet headers without the
 * host touching an address.  What stays the host's: blocking on the answer
 * (the caller holds the HELD frames for a later round), the spare buffers, the
 * TX ring.
 *
 * The cache is an opaque device table of wc_neigh_tab_bytes(cap) = 64 + 32 cap
 * bytes (a 64-byte header, 32-byte entries), 16-byte aligned: open-addressed,
 * of fixed capacity, and it never deletes (the reference never does, short of
 * free_neighbor); a second wc_neigh_tab_init is the flush.  cap is a power of
 * two in [64, 2^20]; any other cap is WC_EINVAL, or 0 bytes.  Sizing the table
 * so that it stays at most half full is the caller's job.
 * Ordering: calls that use one table (init, apply, resolve) are ordered by the
 * caller -- the same stream, or events; an apply and a resolve of one table must
 * not run at once. */
#define WC_NEIGH_TAB_MIN_CAP 64u
#define WC_NEIGH_TAB_MAX_CAP (1u << 20)
uint64_t wc_neigh_tab_bytes(uint32_t cap);                       /* 0 for a bad cap */
/* Asynchronous on `stream`, one launch.  WC_EINVAL: a bad cap, a NULL or not
 * 16-byte-aligned d_tab. */
int wc_neigh_tab_init(void *d_tab, uint32_t cap, void *stream);

/* neighbor_update for the records j < MIN(*d_count, m) of a wc_rx_neigh_updates
 * array, applied as if in order: afterwards every address a record names maps
 * to the MAC of the last record that names it, and every address that was in
 * the table and is not named keeps its MAC.  Records with af 0 (the empty ones)
 * are skipped; an af other than 0 / 4 / 6 is skipped and counted in *d_dropped.
 * The key is (af, addr); for af 4 only addr bytes 0..3 count, and af 4 a.b.c.d
 * and af 6 a.b.c.d:: are different keys.  A record whose key is neither present
 * nor insertable (the table is full) is dropped and counted: the keys present
 * afterwards are the old ones plus MIN(free entries, new distinct keys) of the
 * new ones -- which of them is unspecified --, every key present has the MAC of
 * its last record, and *d_dropped (device uint64, optional, accumulated) counts
 * the records whose key is not present.
 * The result, read through lookups, is the same for the same input however the
 * lanes interleave (but for which new keys a full table keeps); no lane waits for another's store (no spin, no lock), every
 * loop is bounded by cap; two launches, asynchronous on `stream`; atomics only
 * on the table's own words and on *d_dropped (one per workgroup).  d_scratch:
 * wc_neigh_apply_scratch(m) = 4 m bytes of device memory, the caller's, one per
 * call in flight.  cap is read from the table's header on the device; a table
 * that was never initialised is the caller's error (the device then applies
 * nothing and counts every record as dropped, where it can tell).
 * m = 0 is WC_OK and looks at no pointer.  WC_EINVAL, before a device is
 * touched: with m > 0 a NULL d_tab / d_upd / d_count / d_scratch, d_tab not
 * 16-byte or d_upd / d_scratch not 4-byte aligned, m > 2^31. */
uint64_t wc_neigh_apply_scratch(uint32_t m);
int wc_neigh_apply(void *d_tab, const struct wc_neigh_update *d_upd, const uint64_t *d_count,
                   uint32_t m, uint64_t *d_dropped, void *d_scratch, void *stream);

/* Pure host arithmetic over a host copy of the table (no GPU, no library
 * state), like wc_rx_socktab_lookup: the same hash and probe the device runs.
 * Lookup: 1 and mac written for a hit, 0 for a miss; WC_EINVAL for a NULL or not
 * 4-byte-aligned h_tab, bytes wc_neigh_tab_init did not write, a NULL addr /
 * mac, an af other than 4 / 6 (af 4: 4 address bytes are read).  Stats: the
 * capacity and the number of entries in use (either pointer may be NULL). */
int wc_neigh_tab_lookup(const void *h_tab, uint8_t af, const uint8_t *addr, uint8_t mac[6]);
int wc_neigh_tab_stats(const void *h_tab, uint32_t *cap, uint32_t *used);

/* The batched who_has over a destination table.  struct wc_tx_dst has no family
 * field, so d_af[k] (4 or 6) says how d_dsts[k].addr is read.  Per entry k <
 * ndst, d_state[k] is:
 *   READY     neighbor_find (neighbor.c:75-82) gave a MAC that is not
 *             ff:ff:ff:ff:ff:ff: it is written to d_dsts[k].dmac.
 *   BAD_AF    d_af[k] is not 4 / 6: the entry is untouched.
 *   MISS / MISS_DUP   no entry, or a cached broadcast MAC (who_has treats it as
 *             unresolved, neighbor.c:102): dmac is written ff x 6, what
 *             neighbor_find returns; MISS for the lowest index k with that (af,
 *             address) among the array's misses, MISS_DUP for the others -- one
 *             solicitation per distinct unresolved address, the batch form of
 *             the reference's blocking loop, in which a second send to the same
 *             address finds it resolved.
 * addr, port and every byte outside dmac are never written.  With d_list /
 * d_count (both or neither): wc_rx_select(d_state, ndst, WC_NR_MASK_SOLICIT,
 * ...) behind it, ascending.  The de-duplication has wc_neigh_apply's contract:
 * "lowest index wins" whatever the interleaving, no waiting, bounded loops,
 * atomics only on d_scratch's words.  d_scratch: wc_tx_resolve_scratch(ndst)
 * bytes (0 for ndst = 0 or > 65536), 4-byte aligned, needed with or without a
 * list.  ndst = 0 is WC_OK and writes a 0 count if one is given.  WC_EINVAL: a
 * list without its count or a count without its list, ndst > 65536 (the
 * build's limit), a NULL d_tab / d_dsts / d_af / d_state / d_scratch, d_tab not
 * 16-byte or d_dsts / d_scratch not 4-byte aligned.  Asynchronous on `stream`:
 * a memset and two launches, three more with the list. */
enum wc_neigh_resolve {          /* uint8, all < 32 so wc_rx_select masks apply */
    WC_NR_READY = 0,             /* in the cache: dmac written */
    WC_NR_BAD_AF = 4,            /* d_af[k] is not 4 / 6: entry untouched */
    WC_NR_MISS = 8,              /* not in the cache, first entry of the array with this address: solicit */
    WC_NR_MISS_DUP = 9,          /* not in the cache, an earlier entry has the same (af, address) */
};
#define WC_NR_MASK_SOLICIT (0x100u)
#define WC_NR_MASK_MISS    (0x300u)
uint64_t wc_tx_resolve_scratch(uint32_t ndst);
int wc_tx_resolve(const void *d_tab, struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
                  uint8_t *d_state, uint32_t *d_list, uint64_t *d_count, void *d_scratch, void *stream);

/* What the host would otherwise work out per frame from d_state: d_hold[i] by
 * this chain over frame i's descriptor, first hit wins.
 *   1. sock >= ns, or the socket's af is not 4 / 6:     MALFORMED (the build's check 1).
 *   2. a connected socket:                              READY.
 *   3. dst >= ndst, or d_af[dst] is not the socket's af: MALFORMED.
 *   4. d_state[dst] == WC_NR_READY:                     READY.
 *   5. otherwise:                                       HELD.
 * With d_list / d_count (both or neither): wc_rx_select(d_hold, n,
 * WC_TH_MASK_HELD, ...), d_scratch of wc_rx_select_scratch(n) bytes.  The
 * caller passes the READY frames to wc_tx_build_ragged and keeps the HELD ones
 * for the next round.  n = 0 is WC_OK and writes a 0 count if one is given.
 * WC_EINVAL: a list without its count or the reverse, n > 2^32, ns > 256, ndst
 * > 65536, a NULL or not 8-byte-aligned d_desc, a NULL d_hold, NULL or not
 * 4-byte-aligned d_socks with ns > 0, NULL d_state / d_af with ndst > 0, a list
 * without a 4-byte-aligned d_scratch.  One launch, three more with the list;
 * no atomic. */
enum wc_tx_hold { WC_TH_READY = 0, WC_TH_MALFORMED = 4, WC_TH_HELD = 8 };
#define WC_TH_MASK_HELD (0x100u)
int wc_tx_hold_plan(const struct wc_tx_desc *d_desc, uint64_t n, const struct wc_tx_sock *d_socks, uint32_t ns,
                    const uint8_t *d_state, const uint8_t *d_af, uint32_t ndst,
                    uint8_t *d_hold, uint32_t *d_list, uint64_t *d_count, void *d_scratch, void *stream);

/* The contract of wc_rx_neigh_build for wc_tx_resolve's d_list / d_count: frame
 * j < MIN(*d_count, m) solicits d_dsts[d_list[j]], is written at d_out_base +
 * d_out_off[j] and d_out_len[j] is its length; *d_built is written, not
 * accumulated.  d_out_len[j] is 0 and the slot untouched where the index is >=
 * ndst, d_af is not 4 / 6, slot_bytes is below 42 / 86, j is at or past the
 * count, or the engine table has no entry of that family (no af-4 entry; entry
 * 0 not af 6) -- a deliberate difference: the reference would read an unset
 * ifaddr[addr4_pos] / ifaddr[0] there.  Nothing outside [slot, slot + length)
 * is written; all stores are plain vector stores.
 *   ARP who-has, 42 bytes (arp.c:107-142): dst ff x 6, src = mac, 08 06; 00 01
 *     08 00 06 04 00 01; sha = mac, spa = the first af-4 entry's address, tha =
 *     00 x 6, tpa = addr[0..3].
 *   Neighbour solicitation, 86 bytes (icmp6.c:85-129, 60-78; ip6.c:127-161;
 *     ip6.h:61-67, 154-158): dst 33 33 then target bytes 12..15 (the
 *     reference's form, not RFC 2464's 33 33 ff), src = mac, 86 dd; 60 00 00 00
 *     (written whole, as the existing replies), 00 20, 3a, ff, src = entry 0's
 *     address, dst = ff 02 00 .. 00 01 ff then target bytes 13..15; 87 00,
 *     checksum, 60 00 00 00 (the reference sets id = 0x60 on a solicitation
 *     too; the quirk is kept), the 16 target bytes, 01 01, mac.  Checksum:
 *     payload_cksum(ip, 72) with the field taken as 0, stored raw.
 * m = 0 is WC_OK, writes *d_built = 0 and looks at no other pointer; ndst = 0
 * writes that and m zero lengths.  WC_EINVAL: as wc_rx_neigh_build (ndst in
 * the place of n, at most 65536; d_dsts and d_eng 4-byte aligned).  The only
 * atomic is the built count's, one per workgroup of a grid no larger than the
 * device holds at once. */
int wc_tx_solicit_build(const struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
                        const uint32_t *d_list, const uint64_t *d_count, const struct wc_rx_engine *d_eng,
                        void *d_out_base, const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                        uint16_t *d_out_len, uint64_t *d_built, void *stream);

/* --- TX pump: the whole per-batch TX plan and build in one call ------------ */

/* A TX burst is a ring's worth of frames to a few hundred destinations, and at
 * that size wc_tx_resolve -> wc_tx_hold_plan -> wc_tx_solicit_build ->
 * wc_tx_build_ragged costs a memset and eleven launches and nothing else -- and
 * between the hold plan and the build the caller had to read d_hold back and
 * compact the READY frames by hand, because the build takes no hold array.
 * wc_tx_pump is that chain as one call with the build gated on the device: for
 * n <= WC_TX_PUMP_SMALL frames and ndst <= WC_TX_PUMP_SMALL_DST destinations --
 * with m <= WC_TX_PUMP_SMALL_DST solicitation slots: more than such a batch's
 * destinations can fill take the other path, where a grid zeroes them -- it
 * is TWO launches (one workgroup for the destinations, both lists and the
 * solicitations; then one wave per 64 frames for the build); for a larger batch
 * it issues the three calls itself and then the same gated build, so a caller
 * has one entry point for any batch and no host round trip in either.
 *
 * The contract: for every n, ndst and m, every output -- the six dmac bytes of
 * every d_dsts entry included -- holds exactly the bytes this sequence leaves:
 *   wc_tx_resolve(d_tab, d_dsts, d_af, ndst, state, miss_list, miss_count, d_scratch, st);
 *   wc_tx_hold_plan(d_desc, n, d_socks, ns, state, d_af, ndst, hold, held_list, held_count, d_scratch, st);
 *   wc_tx_solicit_build(d_dsts, d_af, ndst, miss_list, miss_count, d_eng, d_sol_base, d_sol_off, m,
 *                       sol_slot_bytes, sol_len, sol_built, st);
 *   the gated build, per frame i:
 *     hold[i] == WC_TH_READY      everything wc_tx_build_ragged does for that frame with the same
 *                                 tables, slot_bytes and flags: the headers, frame_len, status, the
 *                                 two optional values, its share of *errors.
 *     hold[i] == WC_TH_MALFORMED  the frame is untouched, frame_len 0, status WC_TX_MALFORMED, and it
 *                                 is counted in *errors.  Stricter than the build alone where
 *                                 d_af[dst] is not the socket's family: the build would write that
 *                                 frame, the pump refuses it.
 *     hold[i] == WC_TH_HELD       the frame is untouched, frame_len 0, status WC_TX_PUMP_HELD, and it
 *                                 is NOT counted in *errors.
 *   Under both non-READY codes out_ip_hdr[i] and out_udp[i] are 0 where the arrays are given, and no
 *   payload byte of the frame is read.
 * WC_TX_PUMP_HELD is not an enum wc_tx_status code, and WC_TX_IS_ERROR is true
 * for it: test hold[i] (or the held list) before applying the macro to a pump
 * status.  List entries at and past a count keep what they held; the three
 * counts are written, *errors is accumulated; nothing outside a frame or a
 * solicitation slot is read or written; the same input gives the same output.
 * The table is only read, and wc_tx_resolve's ordering rule against
 * wc_neigh_apply carries over.  The frames and the solicitation slots must not
 * overlap.  flags: WC_TX_ZERO_UDP_CKSUM or 0.
 *
 * Every member of *out is a device pointer with the size and alignment its call
 * above asks for (state, miss_list: ndst entries; hold, held_list, frame_len,
 * status, out_ip_hdr, out_udp: n; sol_len: m; the counts: 1).  out_ip_hdr,
 * out_udp and errors are optional.  d_scratch: wc_tx_pump_scratch(n, ndst) bytes
 * of device memory, 4-byte aligned, the caller's, one per call in flight --
 * enough for the calls above, which share it.  The function is pure arithmetic:
 * 0 for (0, 0) and for ndst > 65536, never decreasing in either argument.
 *
 * Empty sides are WC_OK.  n = 0: no frame-side pointer is looked at, *held_count
 * is written 0.  ndst = 0: no destination-side pointer is looked at, *miss_count
 * is written 0, *sol_built 0 and m zero lengths.  m = 0: no solicitation
 * pointer is looked at but sol_built.
 * WC_EINVAL, before a device is touched: a NULL out, a NULL miss_count /
 * held_count / sol_built; n > 2^32, ns > 256, ndst > 65536; slot_bytes or
 * sol_slot_bytes > 65535; a flag bit other than WC_TX_ZERO_UDP_CKSUM
 * (WC_TX_NO_STORE included); and with the respective side non-empty every NULL
 * or misaligned pointer its chain call refuses (a list is always asked for),
 * which includes a NULL or not 4-byte-aligned d_scratch whenever n > 0 or ndst
 * > 0, and a NULL sol_len with m > 0.  Asynchronous on `stream`, no library
 * lock.  The two launches: no workgroup waits for another, nothing spins, every
 * loop is bounded by n, ndst, m, the table's cap or the set's size; all global
 * stores are plain vector stores, and the only global atomic is the error
 * count's, one per wave with an error. */
#define WC_TX_PUMP_SMALL     4096u   /* frames        */
#define WC_TX_PUMP_SMALL_DST 4096u   /* destinations  */
#define WC_TX_PUMP_HELD      0x80u   /* d_status of a HELD frame; not an enum wc_tx_status code */

struct wc_tx_pump_out {              /* host struct of device pointers */
    uint8_t *state;  uint32_t *miss_list;  uint64_t *miss_count;     /* as wc_tx_resolve   (ndst, ndst, 1) */
    uint8_t *hold;   uint32_t *held_list;  uint64_t *held_count;     /* as wc_tx_hold_plan (n, n, 1)       */
    uint16_t *sol_len;  uint64_t *sol_built;                         /* as wc_tx_solicit_build (m, 1)      */
    uint16_t *frame_len;  uint8_t *status;                           /* as wc_tx_build_ragged (n, n)       */
    uint16_t *out_ip_hdr;  uint16_t *out_udp;  uint64_t *errors;     /* optional; errors accumulated       */
};
uint64_t wc_tx_pump_scratch(uint64_t n, uint32_t ndst);
int wc_tx_pump(const void *d_tab, struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
               const struct wc_tx_desc *d_desc, uint64_t n, const struct wc_tx_sock *d_socks, uint32_t ns,
               void *d_base, const uint64_t *d_off, uint32_t slot_bytes, uint32_t flags,
               const struct wc_rx_engine *d_eng, void *d_sol_base, const uint64_t *d_sol_off, uint32_t m,
               uint32_t sol_slot_bytes, const struct wc_tx_pump_out *out, void *d_scratch, void *stream);

/* --- host-memory batch (end-to-end: pinned H2D, kernel, D2H) ------------- */

/* Same as wc_cksum_ragged, but every buffer is host memory: packet i is
 * h_len[i] bytes at h_base + h_off[i], inside [h_base, h_base + h_bytes)
 * (WC_EINVAL otherwise), in any order.  Synchronous; results land in h_out.
 *   - Registered region (wc_host_register), up to 256 packets: the resident
 *     server grid answers (no launch); up to 4096 packets and 8 MiB: one
 *     kernel reads the packets in place over PCIe -- the low-latency path for
 *     a socket or ring batch.
 *   - Registered, larger, and sparse (the packets cover < 7/8 of their byte
 *     range: netmap slots) or out of order: kernels read the packets in place,
 *     64 K packets per launch -- only the lines they touch cross the link.
 *   - Otherwise chunks are streamed over several HIP streams with
 *     hipMemcpyAsync: dense ascending offsets ship the byte range a chunk
 *     covers (DMA straight from a registered region), anything else is
 *     gathered packet by packet into the library's pinned staging first. */
int wc_cksum_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                  const uint16_t *h_len, uint64_t n, uint16_t *h_out, int kind);

/* The fused TX pair over host-memory IP packets (each at its IP header, len =
 * IP header + UDP length, as udp_tx hands them to payload_cksum):
 * h_out_payload[i] = payload_cksum(pkt, len) and h_out_ip_hdr[i] =
 * ip_cksum(pkt, ip4_hl(pkt[0])) for IPv4 (0 for IPv6) -- the two checksums
 * mk_ip4_hdr and udp_tx compute per iov inside w_tx's loop (ip4.c:184-186,
 * udp.c:209-213, backend_netmap.c:348-358), for a whole w_iov_sq in one
 * call, one read of each packet's bytes.  Both fields must hold 0 in the
 * bytes (as the reference zeroes them before summing); store each result
 * raw.  Same paths and rules as wc_cksum_host: a small registered batch is
 * answered by the resident server or one zero-copy launch, anything else is
 * pipelined.  An IPv4 header (hl bytes, options included) must lie inside
 * [h_base, h_base + h_bytes) even where len is shorter: its checksum is
 * defined whatever len is, and every path reads it whole.  len < hl itself is
 * outside payload_cksum's defined inputs (the reference's len - hl wraps to
 * ~4 GiB, in_cksum.c:164): h_out_payload is then unspecified (no byte past
 * the packet's span is read).  Synchronous. */
int wc_cksum_ip_udp_host(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                         const uint16_t *h_len, uint64_t n, uint16_t *h_out_ip_hdr,
                         uint16_t *h_out_payload);

/* The resident small-batch server's counters since the process started, over
 * every device (any pointer may be NULL): batches it answered, batches it was
 * asked for but could not answer (they took the launch path instead), and
 * grid launches. */
int wc_server_stats(uint64_t *served, uint64_t *fallbacks, uint64_t *launches);

/* Quiesce the resident server.  While its grid is resident (it stays up while
 * small registered calls keep coming, and for WC_SERVE_IDLE_US -- 20 ms --
 * after the last), a device-wide synchronisation in the same process
 * (hipDeviceSynchronize, torch.cuda.synchronize()) waits for it: under steady
 * small-batch traffic, with no end.  wc_server_pause stops the grid on every
 * device and returns once no wave of it is left; until the matching
 * wc_server_resume, small registered batches take the zero-copy launch
 * instead (the same results, ~10 us more per call).  Pauses nest: the server
 * serves again after as many resumes as pauses.  wc_server_resume without a
 * pause is WC_EINVAL.  Callable from any thread. */
int wc_server_pause(void);
int wc_server_resume(void);

/* Page-lock a host region (e.g. the netmap buffer area w->mem,
 * backend_netmap.c:149-151) so wc_cksum_host can DMA from it directly.
 * Registering the same base again drops the old registration and pins the
 * pages mapped there now, at the new size (if that fails, the old range is
 * pinned again and the error returned).  Call wc_host_unregister before
 * freeing a registered region: a batch over a freed and re-allocated range
 * that was not registered again reads the pages pinned before the free. */
int wc_host_register(void *h_ptr, uint64_t bytes);
int wc_host_unregister(void *h_ptr);

/* --- multi-GPU batches (one host thread, G devices) ----------------------- */

/* The batch shards across the GPUs of one node as an even contiguous split
 * of packet indices: shard g of G holds packets
 * [g*n/G, (g+1)*n/G).  Packets are independent, so no data moves between
 * GPUs during the checksum; RCCL over xGMI is used only to gather the 2-byte
 * results afterwards, if the caller wants them on every device.  Everything
 * below is callable from warpcore's single engine thread (README.md:24-28). */

/* Set up G shard executors, one per device: devices[g], or device g when
 * `devices` is NULL (ngpus <= 0: every visible device).  A device may be
 * listed more than once (shards then share it; rehearsal on fewer GPUs).
 * Creates each device's scratch, streams and pinned staging.  The caller's
 * current device is left unchanged. */
int wc_gpu_init_multi(int ngpus, const int *devices);
/* Number of shard executors set up by wc_gpu_init_multi (0 before). */
int wc_gpu_multi_count(void);

/* The even contiguous split: packets [*lo, *hi) of n go to shard g of G.
 * Pure arithmetic (no GPU); the split every *_multi call uses. */
int wc_shard_range(uint64_t n, int g, int ngpus, uint64_t *lo, uint64_t *hi);

/* wc_cksum_host over the G shard devices: shard g's packets are copied to
 * and checksummed on its own device (its own PCIe link and copy engines),
 * the devices' pipelines interleaved by the calling thread; results land in
 * h_out in packet order.  Synchronous.  A region registered with
 * wc_host_register is DMA'd directly by every device.  A small registered
 * batch (the zero-copy size of wc_cksum_host) runs on shard 0 alone.
 * Before wc_gpu_init_multi this is wc_cksum_host on the current device. */
int wc_cksum_host_multi(const void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                        const uint16_t *h_len, uint64_t n, uint16_t *h_out, int kind);

/* Device-resident shards: shard g (g < wc_gpu_multi_count()) is the batch
 * d_base[g] (+ d_off[g] / d_len[g]) of n[g] packets on shard g's device,
 * results into d_out[g] on that device, enqueued on streams[g] (streams may
 * be NULL: each device's default stream).  Asynchronous, like the
 * single-device calls. */
int wc_cksum_strided_multi(const void *const *d_base, uint64_t stride, uint16_t len,
                           const uint64_t *n, uint16_t *const *d_out, int kind,
                           void *const *streams);
int wc_cksum_ragged_multi(const void *const *d_base, const uint64_t *const *d_off,
                          const uint16_t *const *d_len, const uint64_t *n,
                          uint16_t *const *d_out, int kind, void *const *streams);

/* After the shards: every shard device g receives all Σn results in packet
 * order in d_all[g] (shard h at offset Σ n[<h]) -- RCCL over xGMI, one
 * ncclBroadcast per shard in one group, on communicators the library creates
 * at the first call (ncclCommInitAll over the shard devices, which must be
 * distinct) and frees in wc_gpu_fini.  Enqueued on streams[g]; RCCL is
 * loaded at run time (WC_ECOMM if it is missing). */
int wc_gather_results_multi(uint16_t *const *d_shard_out, const uint64_t *n,
                            uint16_t *const *d_all, void *const *streams);

/* --- library lifetime / introspection ------------------------------------ */

/* Select the HIP device for this thread and create the library's scratch
 * (staging ring, streams).  Called implicitly by every entry point with
 * device -1 ("current device"); calling it explicitly is optional. */
int wc_gpu_init(int device);
/* Release the scratch created by wc_gpu_init / wc_gpu_init_multi and the
 * RCCL communicators.  Page-locks taken with wc_host_register are the
 * caller's and stay until wc_host_unregister.  Every other entry point may
 * be called from any thread at any time, but not while wc_gpu_fini runs:
 * the caller quiesces its engine threads first. */
int wc_gpu_fini(void);

/* The WC_* environment is read once, at the first initialisation.  This
 * (shipped) library reads only the resident server's WC_SERVE (0: off),
 * WC_SERVE_IDLE_US, WC_SERVE_WAVES and WC_SERVE_MAX, and the staging pool's
 * WC_STAGE_THREADS; its kernel shapes and path choices are a compile-time
 * table.  The tuning build (libwccksum_tune.so, -DWC_TUNING) also reads every
 * path knob.  Re-read the environment now. */
int wc_config_reload(void);

/* Counter-based synthetic packet bytes (bench / tests): little-endian 8-byte
 * word k of [d_buf, d_buf + nbytes) is splitmix64 output k for `seed`. */
int wc_synth_fill(void *d_buf, uint64_t nbytes, uint64_t seed, void *stream);

/* Shader-clock probe (bench / tools): one wave on `stream` writes n pairs
 * (100-MHz wall clock, shader clock counter) to d_samples[2 i], [2 i + 1],
 * one pair every `interval` wall-clock ticks, then ends.  Run beside a
 * timed workload on another stream; the ratio of successive deltas x 100 is
 * the shader clock in MHz while it ran. */
int wc_sclk_probe(uint64_t *d_samples, int n, uint64_t interval, void *stream);

/* Kernel-configuration introspection: fills the group width G (lanes per
 * packet), chunk loads per lane and packets per group-iteration the
 * dispatcher picks for a strided batch of `len`-byte packets. */
int wc_plan_strided(uint64_t base_addr, uint64_t stride, uint16_t len,
                    uint64_t n, int kind, int *group, int *chunks_per_lane,
                    int *unroll, int *grid);

/* Which kernel family the dispatcher picks for that strided batch: "lean"
 * (aligned, one pass per packet), "group" (group-per-packet) or "seg"
 * (segmented-prefix stream of a packed batch). */
const char *wc_plan_strided_kernel(uint64_t base_addr, uint64_t stride, uint16_t len,
                                   uint64_t n, int kind);

/* Both of the above for the fused call: the shape and the kernel family the
 * dispatcher picks for wc_cksum_ip_udp_strided on that batch (payload_cksum
 * with the header pass on, which takes neither the seg nor the lean route). */
const char *wc_plan_strided_fused(uint64_t base_addr, uint64_t stride, uint16_t len,
                                  uint64_t n, int *group, int *chunks_per_lane,
                                  int *unroll, int *grid);

const char *wc_strerror(int err);
const char *wc_version(void);

#ifdef __cplusplus
}
#endif
