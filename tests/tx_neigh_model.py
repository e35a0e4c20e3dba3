"""What the TX neighbour calls must decide and write, restated for the tests
from the reference, byte by byte and on its own (not from
warpcore_amd/csrc/wc_tx_neigh.h): the neighbour cache as a dict (neighbor.c:48-82),
who_has's lookup over a destination table (neighbor.c:95-118), the per-frame
hold chain, and the frames of arp_who_has (arp.c:107-142) and icmp6_nsol
(icmp6.c:85-129 with mk_icmp6_pkt_hdrs, icmp6.c:60-78, mk_ip6_hdr(v, 0),
ip6.c:127-161, and ip6_mk_snma, ip6.h:154-158).  The checksum comes from the C
oracle's payload_cksum (pinned to the reference's object)."""
from __future__ import annotations

import numpy as np

import rx_reply_model as rr
from oracle import c_oracle

READY, BAD_AF, MISS, MISS_DUP = 0, 4, 8, 9
MASK_SOLICIT, MASK_MISS = 0x100, 0x300
TH_READY, TH_MALFORMED, TH_HELD = 0, 4, 8
MASK_HELD = 0x100
BCAST = b"\xff" * 6
ARP_LEN, NSOL_LEN = 42, 86

# struct wc_neigh_update / wc_tx_dst / wc_tx_sock / wc_tx_desc, stated here on their own
UPDATE = np.dtype([("af", "u1"), ("action", "u1"), ("mac", "u1", 6), ("addr", "u1", 16)])
DST = np.dtype([("addr", "u1", 16), ("dmac", "u1", 6), ("port", "<u2")])
SOCK = np.dtype([("af", "u1"), ("flags", "u1"), ("lport", "<u2"), ("rport", "<u2"),
                 ("smac", "u1", 6), ("dmac", "u1", 6), ("pad", "u1", 2),
                 ("laddr", "u1", 16), ("raddr", "u1", 16)])
DESC = np.dtype([("data_len", "<u2"), ("ip_id", "<u2"), ("sock", "u1"), ("tos", "u1"),
                 ("dst", "<u2")])


def key(af: int, addr: bytes):
    """(af, addr): for af 4 only bytes 0..3 count."""
    addr = bytes(addr)
    return (af, addr[:4]) if af == 4 else (af, addr[:16])


def records(items) -> np.ndarray:
    """[(af, mac, addr)] -> an UPDATE array (af 4: addr padded with zeros)."""
    out = np.zeros(len(items), UPDATE)
    for r, (af, mac, addr) in zip(out, items):
        r["af"] = af
        r["mac"] = np.frombuffer(bytes(mac), np.uint8)
        a = bytes(addr)
        r["addr"][:len(a)] = np.frombuffer(a, np.uint8)
    return out


def apply(cache: dict, upd: np.ndarray, count: int, m: int, cap: int = None) -> int:
    """neighbor_update for records j < min(count, m), in order; the number
    dropped.  With `cap`, a new key finds no room once the dict holds cap keys
    (the in-order form of the full-table rule: the device may keep another
    subset of the new keys, of the same size)."""
    dropped = 0
    u = upd.reshape(-1).view(UPDATE).reshape(-1)
    for j in range(min(count, m)):
        af = int(u["af"][j])
        if af == 0:
            continue
        if af not in (4, 6):
            dropped += 1
            continue
        k = key(af, bytes(u["addr"][j]))
        if k not in cache and cap is not None and len(cache) >= cap:
            dropped += 1
            continue
        cache[k] = bytes(u["mac"][j])
    return dropped


def find(cache: dict, af: int, addr: bytes) -> bytes:
    """neighbor_find: the MAC, or ff x 6."""
    return cache.get(key(af, addr), BCAST)


def resolve(cache: dict, dsts: np.ndarray, afs):
    """(state codes, the dsts array afterwards, the solicit list)."""
    d = dsts.copy().reshape(-1).view(DST).reshape(-1)
    state = np.zeros(d.size, np.uint8)
    seen = set()
    for k in range(d.size):
        af = int(afs[k])
        if af not in (4, 6):
            state[k] = BAD_AF
            continue
        kk = key(af, bytes(d["addr"][k]))
        mac = cache.get(kk, BCAST)
        d["dmac"][k] = np.frombuffer(mac, np.uint8)
        if mac != BCAST:                                           # neighbor.c:102
            state[k] = READY
        else:
            state[k] = MISS_DUP if kk in seen else MISS
            seen.add(kk)
    return state, d, np.flatnonzero(state == MISS).astype(np.uint32)


def hold(descs: np.ndarray, socks: np.ndarray, state, afs):
    """(hold codes, the HELD list) by the chain of wc_tx_hold_plan."""
    de = descs.reshape(-1).view(DESC).reshape(-1)
    so = socks.reshape(-1).view(SOCK).reshape(-1)
    ndst = 0 if state is None else len(state)
    out = np.zeros(de.size, np.uint8)
    for i in range(de.size):
        s, t = int(de["sock"][i]), int(de["dst"][i])
        if s >= so.size or int(so["af"][s]) not in (4, 6):
            out[i] = TH_MALFORMED
        elif int(so["flags"][s]) & 1:
            out[i] = TH_READY
        elif t >= ndst or int(afs[t]) != int(so["af"][s]):
            out[i] = TH_MALFORMED
        else:
            out[i] = TH_READY if int(state[t]) == READY else TH_HELD
    return out, np.flatnonzero(out == TH_HELD).astype(np.uint32)


def _first(eng, af: int):
    for ia in rr._entries(eng):
        if int(ia["af"]) == af:
            return bytes(ia["addr"])
    return None


def solicit(af: int, addr: bytes, eng):
    """The frame that asks for `addr`, or None: an af other than 4 / 6, or an
    engine table without an address of the family to ask from (for af 6 the
    source is entry 0's address, ip6.c:155, so entry 0 must be an af-6 one)."""
    e = eng.reshape(-1)[0]
    mac = bytes(e["mac"])
    addr = bytes(addr)
    if af == 4:
        spa = _first(eng, 4)                                       # ifaddr[addr4_pos], arp.c:132
        if spa is None:
            return None
        return (BCAST + mac + b"\x08\x06" + b"\x00\x01\x08\x00\x06\x04\x00\x01" +
                mac + spa[:4] + bytes(6) + addr[:4])               # arp.c:121-134
    if af != 6:
        return None
    ents = rr._entries(eng)
    if not len(ents) or int(ents[0]["af"]) != 6:
        return None
    tgt = addr[:16]
    icmp = b"\x87\x00\x00\x00" + b"\x60\x00\x00\x00" + tgt + b"\x01\x01" + mac  # icmp6.c:99-111
    snma = bytes.fromhex("ff0200000000000000000001ff") + tgt[13:16]          # ip6.h:154-158
    ip = (b"\x60\x00\x00\x00" + len(icmp).to_bytes(2, "big") + b"\x3a\xff" +
          bytes(ents[0]["addr"]) + snma)
    ck = c_oracle.payload_cksum(ip + icmp, 40 + len(icmp))         # icmp6.c:72-73
    return (b"\x33\x33" + tgt[12:16] + mac + b"\x86\xdd" + ip + icmp[:2] + rr._le16(ck) +
            icmp[4:])                                              # icmp6.c:122-126


def built(out: np.ndarray, out_offs, slot_bytes: int, dsts: np.ndarray, afs, lst, count: int, eng):
    """The output buffer, the lengths and the built count of a solicit build."""
    d = dsts.reshape(-1).view(DST).reshape(-1)
    out = out.copy()
    m = len(out_offs)
    out_len = np.zeros(m, np.uint16)
    for j in range(min(m, count)):
        i = int(lst[j])
        if i >= d.size:
            continue
        fr = solicit(int(afs[i]), bytes(d["addr"][i]), eng)
        if fr is None or len(fr) > slot_bytes:
            continue
        o = int(out_offs[j])
        out[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
        out_len[j] = len(fr)
    return out, out_len, int((out_len != 0).sum())
