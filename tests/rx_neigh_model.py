"""What the RX neighbour calls must decide and write, restated for the tests
from the reference, byte by byte and on its own (not from
warpcore_amd/csrc/wc_rx_neigh.h): eth_rx's ARP branch (eth.c:80-83), arp_rx
(arp.c:157-198) and the is-at frame of arp_is_at (arp.c:65-100), the
neighbour advertisement / solicitation branches of icmp6_rx (icmp6.c:270-322)
and the advertisement icmp6_tx writes (icmp6.c:168-193, 221-228, with
mk_ip6_hdr(v, 0) and icmp6.c:72-73 for the checksum).  The checksum comes from
the C oracle's payload_cksum (pinned to the reference's object); the address
filters are rx_reply_model's."""
from __future__ import annotations

import numpy as np

import rx_reply_model as rr
from oracle import c_oracle

NONE, MALFORMED, UPDATE4, ARP_IS_AT, NADV, UPDATE6 = 0, 4, 8, 9, 10, 11
ALL_ACTIONS = (NONE, MALFORMED, UPDATE4, ARP_IS_AT, NADV, UPDATE6)
REPLIES, UPDATES = (ARP_IS_AT, NADV), (UPDATE4, ARP_IS_AT, NADV, UPDATE6)
MASK_REPLY, MASK_UPDATE = 0x600, 0xF00
HOST = rr.HOST

# struct wc_neigh_update, stated here on its own
UPDATE = np.dtype([("af", "u1"), ("action", "u1"), ("mac", "u1", 6), ("addr", "u1", 16)])


def have_ip4(eng) -> bool:
    return any(int(ia["af"]) == 4 for ia in rr._entries(eng))


def plan_why(fr: bytes, action: int, eng):
    """(code, cause) of the frame `fr` (exactly its flen bytes) with the reply
    plan's action byte: the cause names the line of the chain that decided."""
    flen = len(fr)
    if action != HOST:
        return NONE, "not host"
    if fr[12:14] == b"\x08\x06":                                   # eth.c:80-83
        if not have_ip4(eng):
            return NONE, "no ip4"
        if flen < 42:
            return MALFORMED, "arp short"
        if fr[14:16] != b"\x00\x01" or fr[18] != 6:                # arp.c:161
            return NONE, "arp hw format"
        if fr[16:18] != b"\x08\x00" or fr[19] != 4:                # arp.c:167
            return NONE, "arp proto format"
        if fr[20:22] == b"\x00\x01":                               # arp.c:174-183
            if rr.is_my_ip4(eng, fr[38:42], False):
                return ARP_IS_AT, "request for us"
            return UPDATE4, "request for another"
        if fr[20:22] == b"\x00\x02":                               # arp.c:185-189
            return UPDATE4, "reply"
        return NONE, "arp op"                                      # arp.c:191-193
    if fr[12:14] == b"\x86\xdd":
        if flen < 55 or fr[20] != 58 or fr[54] not in (135, 136):
            return NONE, "not nd"
        if flen < 78:
            return MALFORMED, "nd short"
        if fr[54] == 136:                                          # icmp6.c:270-291
            return UPDATE6, "nadv"
        if rr.is_my_ip6(eng, fr[62:78], False):                    # icmp6.c:312
            return NADV, "nsol for us"
        return NONE, "nsol for another"
    return NONE, "other ethertype"


def plan(fr: bytes, action: int, eng) -> int:
    return plan_why(fr, action, eng)[0]


def _nd_mac(fr: bytes) -> bytes:
    """icmp6.c:272-282, 295-304: the source link-address option, or eth->src."""
    data_len = min(int.from_bytes(fr[18:20], "big"), len(fr) - 62)
    if data_len >= 24 and fr[78] == 1 and fr[79] == 1:
        return fr[80:86]
    return fr[6:12]


def record(fr: bytes, code: int):
    """(af, code, mac, addr) neighbor_update receives, or None: no update code,
    or a frame shorter than the bytes the code reads."""
    if code in (UPDATE4, ARP_IS_AT):
        if len(fr) < 42:
            return None
        return 4, code, fr[22:28], fr[28:32] + bytes(12)          # arp.c:196-197
    if code in (UPDATE6, NADV):
        if len(fr) < 78:
            return None
        addr = fr[62:78] if code == UPDATE6 else fr[22:38]         # icmp6.c:286 / 316-318
        return 6, code, _nd_mac(fr), addr
    return None


def record_bytes(fr: bytes, code: int) -> bytes:
    r = record(fr, code)
    if r is None:
        return bytes(24)
    return bytes((r[0], r[1])) + r[2] + r[3]


def build(fr: bytes, code: int, eng):
    """The reply frame of `code` to the request `fr`, or None."""
    e = eng.reshape(-1)[0]
    mac = bytes(e["mac"])
    if code == ARP_IS_AT:
        if len(fr) < 42:
            return None
        sha, spa, tpa = fr[22:28], fr[28:32], fr[38:42]
        return (sha + mac + b"\x08\x06" + b"\x00\x01\x08\x00\x06\x04\x00\x02" +
                mac + tpa + sha + spa)                             # arp.c:78-96
    if code == NADV:
        if len(fr) < 78:
            return None
        # icmp6.c:173-175 tests ip6_data(buf)[0..1], the ICMPv6 type and code: 135 is
        # never 1, so sla stays 0 and the destination is eth->src (icmp6.c:228)
        icmp = b"\x88\x00\x00\x00" + b"\x60\x00\x00\x00" + fr[62:78] + b"\x02\x01" + mac
        ip = (b"\x60\x00\x00\x00" + len(icmp).to_bytes(2, "big") + b"\x3a\xff" +
              bytes(e["addr"][0]["addr"]) + fr[22:38])
        ck = c_oracle.payload_cksum(ip + icmp, 40 + len(icmp))     # icmp6.c:72-73
        return fr[6:12] + mac + b"\x86\xdd" + ip + icmp[:2] + rr._le16(ck) + icmp[4:]
    return None


class Expect:
    """A batch's expectation through the three calls: codes and causes, the two
    lists, the records of m entries and -- for slots at out_offs -- the out
    lengths, the built count and the whole output buffer."""

    def __init__(self, buf: np.ndarray, offs, lens, actions, eng):
        n = len(offs)
        self.frames = [buf[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() for i in range(n)]
        self.eng = eng
        why = [plan_why(fr, int(actions[i]), eng) for i, fr in enumerate(self.frames)]
        self.nact = np.array([c for c, _ in why], np.uint8).reshape(n)
        self.why = [w for _, w in why]
        bits = self.nact.astype(np.uint32)
        self.rlist = np.flatnonzero((MASK_REPLY >> bits) & 1).astype(np.uint32)
        self.ulist = np.flatnonzero((MASK_UPDATE >> bits) & 1).astype(np.uint32)

    def census(self):
        """{(code, cause): frames}"""
        out = {}
        for c, w in zip(self.nact.tolist(), self.why):
            out[(c, w)] = out.get((c, w), 0) + 1
        return out

    def updates(self, m: int, nact=None, lst=None) -> np.ndarray:
        nact = self.nact if nact is None else nact
        lst = self.ulist if lst is None else lst
        out = np.zeros((m, 24), np.uint8)
        for j in range(min(m, len(lst))):
            i = int(lst[j])
            if i < len(self.frames):
                out[j] = np.frombuffer(record_bytes(self.frames[i], int(nact[i])), np.uint8)
        return out

    def built(self, out: np.ndarray, out_offs, slot_bytes: int, nact=None, lst=None):
        nact = self.nact if nact is None else nact
        lst = self.rlist if lst is None else lst
        out = out.copy()
        m = len(out_offs)
        out_len = np.zeros(m, np.uint16)
        for j in range(min(m, len(lst))):
            i = int(lst[j])
            if i >= len(self.frames):
                continue
            r = build(self.frames[i], int(nact[i]), self.eng)
            if r is None or len(r) > slot_bytes:
                continue
            o = int(out_offs[j])
            out[o:o + len(r)] = np.frombuffer(r, np.uint8)
            out_len[j] = len(r)
        return out, out_len, int((out_len != 0).sum())
