// wc_tx_neigh.h -- what the TX neighbour kernels (wc_k_txneigh.hip), the host
// lookup of the runtime (wc_rt_txneigh.cpp) and a host test share, each stated
// once: the neighbour cache as an open-addressed table
// of words with its hash, key compare and the probe / claim / commit steps of
// wc_neigh_apply, the lookup, the resolve and de-duplication steps of
// wc_tx_resolve, the chain of wc_tx_hold_plan, and the 42 bytes of an ARP
// who-has and the 86 bytes of a neighbour solicitation as frame-relative
// dwords.  Plain C++ (no device builtin): the table words, the atomics on them
// and the frame stores go through two small policy parameters, so the kernels
// and a host program compile the same lines.
//   Words: ld / ld8 (plain loads of input nobody writes in the launch), ld_now
//     (a word other lanes change with atomics in this launch), st / st16 / st8,
//     cas(p, expect, want) -> the old word, amax(p, v).
//   Mem:   st8 / st16 / st32(address, value), as txb::store_words takes it.
// The engine table is wc_rx_reply.h's; the 14-byte shift, the folds and the
// stores at any 4-byte phase are wc_tx_build.h's.
//
// Reference decisions and stores restated (read, not copied; paths in the
// reference tree):
//   neighbor_update  lib/src/neighbor.c:48-65    insert or overwrite
//   neighbor_find    lib/src/neighbor.c:75-82    the MAC, or ff x 6
//   who_has          lib/src/neighbor.c:95-118   a broadcast MAC is unresolved
//   arp_who_has      lib/src/arp.c:107-142       the request frame
//   icmp6_nsol       lib/src/icmp6.c:85-129, 60-78   the solicitation
//   mk_ip6_hdr       lib/src/ip6.c:127-161;  ip6_mk_snma  lib/src/ip6.h:154-158
//   payload_cksum    lib/src/in_cksum.c:146-161
#pragma once

#include <stdint.h>
#include <string.h>

#include "wc_rx_reply.h"

namespace wc {
namespace tn {

// The table: a 64-byte header -- h[0] = kTabMagic, h[1] = cap, the rest 0 --
// then cap entries of 32 bytes: e[0] = state, e[1] = last, e[2] = af | mac[0..1]
// << 16, e[3] = mac[2..5], e[4..7] = addr (af 4: e[4] alone, e[5..7] = 0).
// state: kEmpty, kFull, or kClaim | j -- claimed in the running apply by record
// j.  last: 1 + the highest record index that named the entry in the running
// apply; 0 between calls.
constexpr uint32_t kTabMinCap = 64u, kTabMaxCap = 1u << 20; // WC_NEIGH_TAB_*
constexpr uint32_t kTabMagic = 0x4254434Eu;
constexpr uint32_t kHdrWords = 16u, kEntWords = 8u;
constexpr uint32_t kEmpty = 0u, kFull = 1u, kClaim = 0x80000000u;
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;
constexpr uint32_t kApplyMax = 1u << 31; // a claim holds the record index in 31 bits
constexpr uint32_t kUpdWords = 6u;       // struct wc_neigh_update in dwords (wc_rx_neigh.h)

// enum wc_neigh_resolve, enum wc_tx_hold (wc_cksum.h)
constexpr uint32_t kReady = 0, kBadAf = 4, kMiss = 8, kMissDup = 9;
constexpr uint32_t kMaskSolicit = 0x100u, kMaskMiss = 0x300u; // WC_NR_MASK_*
constexpr uint32_t kThReady = 0, kThMalformed = 4, kThHeld = 8;
constexpr uint32_t kMaskHeld = 0x100u; // WC_TH_MASK_HELD
constexpr uint32_t kArpLen = 42u, kNsolLen = 86u;
constexpr uint32_t kResolveMax = 65536u; // the TX build's ndst limit

WC_HD bool cap_ok(uint32_t cap)
{
    return cap >= kTabMinCap && cap <= kTabMaxCap && (cap & (cap - 1u)) == 0u;
}

WC_HD uint64_t tab_bytes(uint32_t cap)
{
    return cap_ok(cap) ? 4ull * kHdrWords + 4ull * kEntWords * cap : 0ull;
}

// (af, addr): af 4 reads addr's first word alone, so 4 / a.b.c.d and 6 /
// a.b.c.d:: are different keys and bytes 4..15 of an af-4 address never count.
struct Key {
    uint32_t af, a[4];
};

WC_HD Key key_of(uint32_t af, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3)
{
    const bool v6 = af == 6u;
    return Key{af, {a0, v6 ? a1 : 0u, v6 ? a2 : 0u, v6 ? a3 : 0u}};
}

WC_HD bool key_eq(const Key &x, const Key &y)
{
    return x.af == y.af && x.a[0] == y.a[0] && x.a[1] == y.a[1] && x.a[2] == y.a[2] &&
           x.a[3] == y.a[3];
}

// A mixed hash over af and the address words (murmur3's steps): the low bits
// of an address alone would put a /24 into 256 neighbouring entries.
WC_HD uint32_t hash(const Key &k)
{
    uint32_t h = 0x9E3779B1u * k.af;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        uint32_t x = k.a[i] * 0xCC9E2D51u;
        x = (x << 15) | (x >> 17);
        h ^= x * 0x1B873593u;
        h = ((h << 13) | (h >> 19)) * 5u + 0xE6546B64u;
    }
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// The table's cap as its header states it; 0 -- every probe loop then runs no
// step -- for words wc_neigh_tab_init did not write.
template <class Words>
WC_HD uint32_t tab_cap(const Words &w, const uint32_t *tab)
{
    const uint32_t magic = w.ld(tab), cap = w.ld(tab + 1);
    return magic == kTabMagic && cap_ok(cap) ? cap : 0u;
}

WC_HD uint32_t *tab_entry(uint32_t *tab, uint32_t s)
{
    return tab + kHdrWords + kEntWords * s;
}

WC_HD const uint32_t *tab_entry(const uint32_t *tab, uint32_t s)
{
    return tab + kHdrWords + kEntWords * s;
}

// The key of record j of a wc_rx_neigh_updates array, and of a full entry.
template <class Words>
WC_HD Key record_key(const Words &w, const uint32_t *upd, uint32_t j)
{
    const uint32_t *u = upd + kUpdWords * j;
    return key_of(w.ld(u) & 0xFFu, w.ld(u + 2), w.ld(u + 3), w.ld(u + 4), w.ld(u + 5));
}

template <class Words>
WC_HD Key entry_key(const Words &w, const uint32_t *e)
{
    return key_of(w.ld(e + 2) & 0xFFu, w.ld(e + 4), w.ld(e + 5), w.ld(e + 6), w.ld(e + 7));
}

// wc_neigh_apply, launch 1, record j < lim: the entry that holds or now claims
// the record's key, with last raised to j + 1; kNoEntry for an empty record (af
// 0), and with `dropped` set for an af other than 4 / 6 and for a key that is
// neither present nor insertable.  A full entry is compared by its own key, a
// claimed one by the key of the record that claimed it -- input nobody writes,
// so nothing has to be published first; an empty one is claimed by one
// compare-and-swap, and where that fails the word it returns is looked at
// instead.  A state only ever goes from empty to claimed here, so every lane
// with one key passes the same entries and ends in the same one, whatever the
// order: no lane waits, and the loop ends after cap steps.
template <class Words>
WC_HD uint32_t apply_claim(const Words &w, uint32_t *tab, uint32_t cap, const uint32_t *upd,
                           uint32_t lim, uint32_t j, bool &dropped)
{
    const Key k = record_key(w, upd, j);
    dropped = k.af != 0u && k.af != 4u && k.af != 6u;
    if (k.af != 4u && k.af != 6u)
        return kNoEntry;
    const uint32_t mask = cap - 1u;
    uint32_t s = hash(k) & mask;
    for (uint32_t p = 0; p < cap; ++p, s = (s + 1u) & mask) {
        uint32_t *e = tab_entry(tab, s);
        uint32_t st = w.ld_now(e);
        bool hit = false;
        if (st == kEmpty) {
            st = w.cas(e, kEmpty, kClaim | j);
            hit = st == kEmpty;
        }
        if (!hit && st == kFull)
            hit = key_eq(k, entry_key(w, e));
        else if (!hit && (st & kClaim) && (st & ~kClaim) < lim)
            hit = key_eq(k, record_key(w, upd, st & ~kClaim));
        if (hit) {
            w.amax(e + 1, j + 1u);
            return s;
        }
    }
    dropped = true;
    return kNoEntry;
}

// Launch 2, record j with the entry launch 1 gave it: the one record whose j +
// 1 is the entry's last writes key, MAC and state = full and resets last.  The
// entry's other records read last as that value or as 0, neither of which is
// theirs, so there is no order to get wrong.
template <class Words>
WC_HD void apply_commit(const Words &w, uint32_t *tab, uint32_t cap, const uint32_t *upd, uint32_t j,
                        uint32_t ent)
{
    if (ent >= cap)
        return;
    uint32_t *e = tab_entry(tab, ent);
    if (w.ld_now(e + 1) != j + 1u)
        return;
    const uint32_t *u = upd + kUpdWords * j;
    const Key k = record_key(w, upd, j);
    w.st(e + 2, w.ld(u) & 0xFFFF00FFu); // af, mac[0..1]: the action byte is not kept
    w.st(e + 3, w.ld(u + 1));
    w.st(e + 4, k.a[0]);
    w.st(e + 5, k.a[1]);
    w.st(e + 6, k.a[2]);
    w.st(e + 7, k.a[3]);
    w.st(e + 1, 0u);
    w.st(e, kFull);
}

// neighbor_find over a table no call is changing: the entry's MAC words (m0 =
// mac[0..3], m1 = mac[4..5]) where the key is present.  Nothing is ever
// deleted, so a key lies in front of the first empty entry of its probes.
template <class Words>
WC_HD bool lookup(const Words &w, const uint32_t *tab, uint32_t cap, const Key &k, uint32_t &m0,
                  uint32_t &m1)
{
    const uint32_t mask = cap - 1u;
    uint32_t s = hash(k) & mask;
    for (uint32_t p = 0; p < cap; ++p, s = (s + 1u) & mask) {
        const uint32_t *e = tab_entry(tab, s);
        const uint32_t st = w.ld(e);
        if (st == kEmpty)
            return false;
        if (st == kFull && key_eq(k, entry_key(w, e))) {
            const uint32_t a = w.ld(e + 2), b = w.ld(e + 3);
            m0 = (a >> 16) | (b << 16);
            m1 = b >> 16;
            return true;
        }
    }
    return false;
}

// wc_tx_resolve's de-duplication set: `slots` words (a power of two, at least
// 2 ndst: never full) that hold 0 or 1 + the index of the destination that
// claimed them, then `slots` words that hold 0 or the highest ~k among the
// destinations k with the claimant's key -- the lowest k.
WC_HD uint32_t set_slots(uint32_t ndst)
{
    uint32_t s = 64u;
    while (s < 2u * ndst)
        s <<= 1;
    return s;
}

template <class Words>
WC_HD Key dst_key(const Words &w, const uint32_t *dsts, const uint8_t *afs, uint32_t k)
{
    const uint32_t *t = dsts + txb::kDstWords * k;
    return key_of(w.ld8(afs + k), w.ld(t), w.ld(t + 1), w.ld(t + 2), w.ld(t + 3));
}

// wc_tx_resolve, launch 1, destination k: READY with dmac written where the
// cache holds a MAC that is not ff x 6; BAD_AF with nothing written; else dmac
// = ff x 6 (what neighbor_find returns), MISS for now, and the key enters the
// set by apply_claim's steps -- a claimed slot is compared by its claimant's
// address words, which nobody writes.  where[k] = the set slot, kNoEntry
// without one.  Only the six dmac bytes of an entry are ever stored.
template <class Words>
WC_HD void resolve_find(const Words &w, const uint32_t *tab, uint32_t cap, uint32_t *dsts,
                        const uint8_t *afs, uint32_t ndst, uint32_t k, uint32_t *set, uint32_t slots,
                        uint8_t *state, uint32_t *where)
{
    const Key key = dst_key(w, dsts, afs, k);
    uint32_t *t = dsts + txb::kDstWords * k;
    w.st(where + k, kNoEntry);
    if (key.af != 4u && key.af != 6u) {
        w.st8(state + k, kBadAf);
        return;
    }
    uint32_t m0 = 0u, m1 = 0u;
    const bool found = lookup(w, tab, cap, key, m0, m1) && !(m0 == 0xFFFFFFFFu && m1 == 0xFFFFu);
    w.st(t + 4, found ? m0 : 0xFFFFFFFFu);
    w.st16(t + 5, found ? m1 : 0xFFFFu);
    w.st8(state + k, found ? kReady : kMiss);
    if (found)
        return;
    const uint32_t mask = slots - 1u;
    uint32_t s = hash(key) & mask;
    for (uint32_t p = 0; p < slots; ++p, s = (s + 1u) & mask) {
        uint32_t c = w.ld_now(set + s);
        bool hit = false;
        if (c == 0u) {
            c = w.cas(set + s, 0u, k + 1u);
            hit = c == 0u;
        }
        if (!hit && c - 1u < ndst)
            hit = c - 1u == k || key_eq(key, dst_key(w, dsts, afs, c - 1u));
        if (hit) {
            w.amax(set + slots + s, ~k);
            w.st(where + k, s);
            return;
        }
    }
}

// Launch 2: a miss that is not the lowest index of its set slot is MISS_DUP.
template <class Words>
WC_HD void resolve_mark(const Words &w, uint32_t k, const uint32_t *set, uint32_t slots,
                        uint8_t *state, const uint32_t *where)
{
    const uint32_t s = w.ld(where + k);
    if (s < slots && w.ld(set + slots + s) != ~k)
        w.st8(state + k, kMissDup);
}

// The chain of wc_tx_hold_plan.  sock_in / dst_in: the descriptor's indices
// lie inside the tables; w0: the socket entry's first word (af | flags << 8);
// dst_af / dst_state: d_af[dst] / d_state[dst], read only where dst_in.
WC_HD uint32_t hold_of(bool sock_in, uint32_t w0, bool dst_in, uint32_t dst_af, uint32_t dst_state)
{
    const uint32_t af = w0 & 0xFFu;
    if (!sock_in || (af != 4u && af != 6u))
        return kThMalformed;
    if ((w0 >> 8) & txb::kSockConnected)
        return kThReady;
    if (!dst_in || dst_af != af)
        return kThMalformed;
    return dst_state == kReady ? kThReady : kThHeld;
}

// The solicitation for the address t (a destination entry's words 0..3) of
// family af, written at da: its length, or 0 with nothing written where af is
// not 4 / 6, slot_bytes is below 42 / 86 or the engine table has no address of
// the family to ask from (no af-4 entry; entry 0 not af 6 -- the IPv6 entries
// come first, ifaddr.c:94-146).
template <class Mem>
WC_HD uint32_t solicit(const Mem &m, const uint32_t (&t)[4], uint32_t af, const uint32_t *e,
                       uint64_t da, uint32_t slot_bytes)
{
    const uint32_t mac0 = e[0], mac1 = e[1] & 0xFFFFu;
    const uint32_t macw = (mac0 >> 16) | (mac1 << 16); // mac[2..5]
    const uint32_t na = rr::eng_naddr(e);
    if (af == 4u) {
        bool have4 = false;
        for (uint32_t k = 0; k < na; ++k)
            have4 = have4 || (rr::eng_entry(e, k)[0] & 0xFFu) == 4u;
        if (!have4 || slot_bytes < kArpLen)
            return 0u;
        const uint32_t spa = rr::eng_src4(e); // ifaddr[addr4_pos] (arp.c:132)
        uint32_t h[11];
        h[0] = 0xFFFFFFFFu;                // arp.c:121-123
        h[1] = 0xFFFFu | (mac0 << 16);
        h[2] = macw;
        h[3] = 0x0608u | (0x0100u << 16);  // 08 06, hrd 00 01
        h[4] = 0x04060008u;                // pro 08 00, hln 6, pln 4
        h[5] = 0x0100u | (mac0 << 16);     // op 00 01, sha
        h[6] = macw;
        h[7] = spa;
        h[8] = 0u;                         // tha 00 x 6
        h[9] = t[0] << 16;
        h[10] = t[0] >> 16;                // tpa
        txb::store_words<11, 11>(m, da, true, h);
        return kArpLen;
    }
    if (af != 6u || na == 0u || (rr::eng_entry(e, 0u)[0] & 0xFFu) != 6u || slot_bytes < kNsolLen)
        return 0u;
    const uint32_t *s = rr::eng_entry(e, 0u) + 1; // entry 0's address (ip6.c:155)
    uint32_t ip[18];
    ip[0] = 0x60u; // the whole word, as the existing replies write it
    ip[1] = 0x2000u | (58u << 16) | (0xFFu << 24); // len 00 20, next header, hop limit
    ip[6] = 0x000002FFu; // ff 02 00 .. 00 01 ff, then target bytes 13..15 (ip6.h:154-158)
    ip[7] = 0u;
    ip[8] = 0x01000000u;
    ip[9] = 0xFFu | (t[3] & 0xFFFFFF00u);
    ip[10] = 0x0087u; // type 135, code 0, checksum 0
    ip[11] = 0x60u;   // icmp->id = 0x60 on a solicitation too (icmp6.c:101)
    ip[16] = 0x0101u | (mac0 << 16); // option 01 01, then mac
    ip[17] = macw;
    // payload_cksum(ip, 72) as in_cksum.c:146-161 forms it; 58 << 24 plus 33
    // words stays below 2^32.
    uint32_t S = (58u << 24) + 0x2000u + txb::words(ip[6]) + txb::words(ip[8]) + txb::words(ip[9]) +
                 txb::words(ip[10]) + txb::words(ip[11]) + txb::words(ip[16]) + txb::words(ip[17]);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        ip[2 + k] = s[k];
        ip[12 + k] = t[k];
        S += txb::words(ip[2 + k]) + txb::words(ip[12 + k]);
    }
    ip[10] |= txb::fold_not16(S) << 16; // icmp6.c:72-73, stored raw
    uint32_t h[22];
    h[0] = 0x3333u | (t[3] << 16); // 33 33, then target bytes 12..15 (icmp6.c:122-126)
    h[1] = (t[3] >> 16) | (mac0 << 16);
    h[2] = macw;
    txb::shift14(0xDD86u, ip, h);
    txb::store_words<22, 22>(m, da, true, h);
    return kNsolLen;
}

// The Words of a host program over memory nobody else touches (the runtime's
// wc_neigh_tab_lookup, a serial test).
struct HostWords {
    uint32_t ld(const uint32_t *p) const { return *p; }
    uint32_t ld_now(const uint32_t *p) const { return *p; }
    uint32_t ld8(const uint8_t *p) const { return *p; }
    void st(uint32_t *p, uint32_t v) const { *p = v; }
    void st16(uint32_t *p, uint32_t v) const // the word's low half (little-endian)
    {
        const uint16_t x = (uint16_t)v;
        memcpy(p, &x, 2);
    }
    void st8(uint8_t *p, uint32_t v) const { *p = (uint8_t)v; }
    uint32_t cas(uint32_t *p, uint32_t expect, uint32_t want) const
    {
        const uint32_t old = *p;
        if (old == expect)
            *p = want;
        return old;
    }
    void amax(uint32_t *p, uint32_t v) const
    {
        if (*p < v)
            *p = v;
    }
};

} // namespace tn
} // namespace wc
