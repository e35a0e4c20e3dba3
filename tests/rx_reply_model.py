"""What the RX reply calls must decide and write, restated for the tests from
the reference's RX path, byte by byte and on its own (not from
warpcore_amd/csrc/wc_rx_reply.h): eth_rx's MAC filter (eth.c:65-67), ip4_rx /
ip6_rx's is_my_ip4 / is_my_ip6 (ip4.c:103, 200-214; ip6.c:98, 173-187), the
unreachables of udp_rx and ip4_rx (udp.c:147-155, ip4.c:133-137), icmp4_rx /
icmp6_rx (icmp4.c:144-196, icmp6.c:250-330) and the frames icmp4_tx / icmp6_tx
write (icmp4.c:56-129, icmp6.c:55-78, 140-231, with mk_ip4_hdr(v, 0) /
mk_ip6_hdr(v, 0)).  Every checksum comes from the C oracle's ip_cksum /
payload_cksum (pinned to the reference's object)."""
from __future__ import annotations

import numpy as np

from oracle import c_oracle

NONE, HOST, FILTERED, ICMP_BAD_CKSUM, MALFORMED, NO_ROOM = range(6)
ECHO4, ECHO6, UNREACH_PORT4, UNREACH_PORT6, UNREACH_PROTO4 = range(8, 13)
REPLIES = (ECHO4, ECHO6, UNREACH_PORT4, UNREACH_PORT6, UNREACH_PROTO4)
ALL_ACTIONS = (NONE, HOST, FILTERED, ICMP_BAD_CKSUM, MALFORMED, NO_ROOM) + REPLIES
MASK_REPLY = 0x1F00
RX_OK, RX_OK_NO_CKSUM, RX_NOT_UDP, RX_NOT_IP = 0, 1, 7, 8
SOCK_UNBOUND = 0xFF

# struct wc_rx_ifaddr / wc_rx_engine, stated here on their own
IFADDR = np.dtype([("af", "u1"), ("pad", "u1", 3), ("addr", "u1", 16), ("bcast", "u1", 16),
                   ("snma", "u1", 16)])
ENGINE = np.dtype([("mac", "u1", 6), ("mtu", "<u2"), ("naddr", "<u4"), ("addr", IFADDR, 16)])


def engine(mac: bytes, mtu: int, addrs, rng=None) -> np.ndarray:
    """One ENGINE record: addrs = [(af, addr, bcast, snma)] in table order,
    the byte strings 4 (af 4) or 16 long; with `rng`, garbage in every ignored
    byte (pad, an IPv4 entry's bytes 4..15 and snma, the entries past naddr)."""
    e = np.zeros(1, ENGINE)
    if rng is not None:
        e.view(np.uint8)[:] = rng.integers(0, 256, ENGINE.itemsize, dtype=np.uint8)
    e["mac"][0] = np.frombuffer(mac, np.uint8)
    e["mtu"], e["naddr"] = mtu, len(addrs)
    for k, (af, a, b, s) in enumerate(addrs):
        ia = e["addr"][0][k]
        ia["af"] = af
        for name, v in (("addr", a), ("bcast", b), ("snma", s)):
            if v is not None:
                ia[name][:len(v)] = np.frombuffer(v, np.uint8)
    return e


def _entries(eng):
    e = eng.reshape(-1)[0]
    return [e["addr"][k] for k in range(int(e["naddr"]))]


def is_my_ip4(eng, ip: bytes, match_bcast: bool) -> bool:
    """ip4.c:200-214: from addr4_pos (the first af-4 entry) to the end."""
    ent = _entries(eng)
    pos = next((k for k, ia in enumerate(ent) if int(ia["af"]) == 4), len(ent))
    for ia in ent[pos:]:
        if ip == bytes(ia["addr"][:4]):
            return True
        if match_bcast and (ip == bytes(ia["bcast"][:4]) or ip == b"\xff" * 4):
            return True
    return False


def is_my_ip6(eng, ip: bytes, match_mcast: bool) -> bool:
    """ip6.c:173-187 over the af-6 entries (the library's deliberate
    difference: the reference's loop also compares the IPv4 entries' bytes)."""
    for ia in _entries(eng):
        if int(ia["af"]) != 6:
            continue
        if ip == bytes(ia["addr"]):
            return True
        if match_mcast and (ip == bytes(ia["snma"]) or ip == bytes(ia["bcast"])):
            return True
    return False


def _be(b: bytes) -> int:
    return int.from_bytes(b, "big")


def _le16(v: int) -> bytes:  # a checksum "stored raw": the native word's bytes
    return bytes((v & 0xFF, v >> 8))


def reply_data(fr: bytes, action: int, mtu: int):
    """The request bytes a reply of `action` carries behind its ICMP header,
    or None where the reference would wrap a length (icmp4.c:91, icmp6.c:202)
    or read a byte past the frame."""
    flen = len(fr)
    if action in (ECHO4, UNREACH_PORT4, UNREACH_PROTO4):
        if flen < 34:
            return None
        hl = (fr[14] & 15) * 4
        if action == ECHO4:
            t = min(_be(fr[16:18]), mtu)                      # icmp4.c:80
            if t < hl + 8 or 14 + t > flen:
                return None
            return fr[14 + hl + 8:14 + t]                     # icmp4.c:89-91
        if flen < 14 + hl + 8:
            return None
        return fr[14:14 + hl + 8]                             # icmp4.c:99
    if flen < 54:
        return None
    if action == ECHO6:
        t = min(_be(fr[18:20]), mtu - 40)                     # icmp6.c:164
        if t < 8 or 54 + t > flen:
            return None
        return fr[62:54 + t]                                  # icmp6.c:201-202
    if flen < 102:
        return None
    return fr[54:102]                                         # icmp6.c:163, 210: from ip6_data(buf)


def build(fr: bytes, action: int, eng, ip_id: int = 0):
    """The reply frame of `action` to the request `fr`, or None where
    reply_data has none."""
    e = eng.reshape(-1)[0]
    data = reply_data(fr, action, int(e["mtu"]))
    if data is None:
        return None
    eth = fr[6:12] + bytes(e["mac"])                          # icmp4.c:122-125
    if action in (ECHO4, UNREACH_PORT4, UNREACH_PROTO4):
        hl = (fr[14] & 15) * 4
        if action == ECHO4:
            icmp = b"\x00\x00\x00\x00" + fr[14 + hl + 4:14 + hl + 8] + data
        else:
            icmp = bytes((3, 3 if action == UNREACH_PORT4 else 2)) + bytes(6) + data
        icmp = icmp[:2] + _le16(c_oracle.ip_cksum(icmp)) + icmp[4:]
        src = next((bytes(ia["addr"][:4]) for ia in _entries(eng) if int(ia["af"]) == 4), bytes(4))
        ip = (b"\x45\x00" + (20 + len(icmp)).to_bytes(2, "big") + _le16(ip_id) + b"\x40\x00" +
              b"\xff\x01" + b"\x00\x00" + src + fr[26:30])
        ip = ip[:10] + _le16(c_oracle.ip_cksum(ip)) + ip[12:]
        return eth + b"\x08\x00" + ip + icmp
    if action == ECHO6:
        icmp = b"\x81\x00\x00\x00" + fr[58:62] + data
    else:
        icmp = b"\x01\x04" + bytes(6) + data
    ip = (b"\x60\x00\x00\x00" + len(icmp).to_bytes(2, "big") + b"\x3a\xff" +
          bytes(e["addr"][0]["addr"]) + fr[22:38])
    ck = c_oracle.payload_cksum(ip + icmp, 40 + len(icmp))    # icmp6.c:72-73
    return eth + b"\x86\xdd" + ip + icmp[:2] + _le16(ck) + icmp[4:]


def _finish(fr: bytes, action: int, eng, slot_bytes: int):
    data = reply_data(fr, action, int(eng.reshape(-1)[0]["mtu"]))
    if data is None:
        return MALFORMED, 0
    ln = (42 if action in (ECHO4, UNREACH_PORT4, UNREACH_PROTO4) else 62) + len(data)
    if ln > slot_bytes:
        return NO_ROOM, 0
    return action, ln


def plan(fr: bytes, verdict: int, sock, eng, slot_bytes: int):
    """(action, reply length) of the frame `fr` (exactly its flen bytes) with
    the RX verdict and socket id (None: no d_sock) the calls in front gave."""
    flen = len(fr)
    if verdict not in (RX_OK, RX_OK_NO_CKSUM, RX_NOT_UDP, RX_NOT_IP):
        return NONE, 0
    mac = bytes(eng.reshape(-1)[0]["mac"])
    if fr[0:6] != mac and fr[0:6] != b"\xff" * 6 and fr[0:2] != b"\x33\x33":
        return FILTERED, 0
    if verdict == RX_NOT_IP:
        return HOST, 0
    v4 = fr[12:14] == b"\x08\x00"
    if not (is_my_ip4(eng, fr[30:34], True) if v4 else is_my_ip6(eng, fr[38:54], True)):
        return FILTERED, 0
    if verdict in (RX_OK, RX_OK_NO_CKSUM):
        if sock is None or sock != SOCK_UNBOUND:
            return NONE, 0
        # udp.c:150-153: the SOURCE address (i->wv_ip4 / wv_ip6), as the reference has it
        if v4:
            if not is_my_ip4(eng, fr[26:30], False):
                return NONE, 0
            return _finish(fr, UNREACH_PORT4, eng, slot_bytes)
        if not is_my_ip6(eng, fr[22:38], False):
            return NONE, 0
        return _finish(fr, UNREACH_PORT6, eng, slot_bytes)
    if v4:
        hl = (fr[14] & 15) * 4
        if fr[23] != 1:
            return _finish(fr, UNREACH_PROTO4, eng, slot_bytes)
        icmp_len = min((_be(fr[16:18]) - hl) & 0xFFFF, flen - 14 - hl)   # icmp4.c:153-154
        if c_oracle.ip_cksum(fr[14 + hl:14 + hl + icmp_len]) != 0:
            return ICMP_BAD_CKSUM, 0
        if fr[14 + hl] != 8:
            return NONE, 0
        return _finish(fr, ECHO4, eng, slot_bytes)
    if fr[20] != 58:
        return NONE, 0
    icmp_len = min(_be(fr[18:20]), flen - 54)                            # icmp6.c:259-261
    if c_oracle.payload_cksum(fr[14:54 + icmp_len], 40 + icmp_len) != 0:
        return ICMP_BAD_CKSUM, 0
    if flen < 55:
        return MALFORMED, 0
    if fr[54] in (135, 136):
        return HOST, 0
    if fr[54] == 128:
        return _finish(fr, ECHO6, eng, slot_bytes)
    return NONE, 0


class Expect:
    """A batch's expectation through both calls: actions, reply lengths, the
    reply list, and -- for m slots at out_offs -- the out lengths, the built
    count and the whole output buffer."""

    def __init__(self, buf: np.ndarray, offs, lens, verdicts, socks, eng, slot_bytes: int):
        n = len(offs)
        self.frames = [buf[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() for i in range(n)]
        self.eng, self.slot_bytes = eng, slot_bytes
        self.action = np.zeros(n, np.uint8)
        self.reply_len = np.zeros(n, np.uint16)
        for i, fr in enumerate(self.frames):
            a, ln = plan(fr, int(verdicts[i]), None if socks is None else int(socks[i]), eng,
                         slot_bytes)
            self.action[i], self.reply_len[i] = a, ln
        self.list = np.flatnonzero((MASK_REPLY >> self.action.astype(np.uint32)) & 1) \
            .astype(np.uint32)

    def built(self, out: np.ndarray, out_offs, ip_ids=None, action=None, lst=None):
        """(out after the build, out lengths, built count) for the slots
        out_offs; `action` / `lst`: other arrays than the plan's own (a stale
        action array: each entry gives length 0 or that action's reply)."""
        action = self.action if action is None else action
        lst = self.list if lst is None else lst
        out = out.copy()
        m = len(out_offs)
        out_len = np.zeros(m, np.uint16)
        for j in range(min(m, len(lst))):
            i = int(lst[j])
            a = int(action[i]) if i < len(self.frames) else NONE
            if a not in REPLIES:
                continue
            r = build(self.frames[i], a, self.eng, 0 if ip_ids is None else int(ip_ids[j]))
            if r is None or len(r) > self.slot_bytes:
                continue
            o = int(out_offs[j])
            out[o:o + len(r)] = np.frombuffer(r, np.uint8)
            out_len[j] = len(r)
        return out, out_len, int((out_len != 0).sum())
