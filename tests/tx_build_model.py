"""What the TX build must write, restated for the tests (wc_cksum.h, "TX
build"): the check chain in its order and the 14 + hl + 8 header bytes field
by field; the two checksum values come from the C oracle's ip_cksum /
payload_cksum (pinned to the reference's object) on the model's own frame with
both fields zero.
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle

SEALED, SEALED_ZERO_UDP, MALFORMED, TRUNCATED = 0, 1, 6, 7
SOCK_CONNECTED, SOCK_ECN = 1, 2

# struct wc_tx_sock / wc_tx_dst / wc_tx_desc, stated here on their own
SOCK = np.dtype([("af", "u1"), ("flags", "u1"), ("lport", "<u2"), ("rport", "<u2"),
                 ("smac", "u1", 6), ("dmac", "u1", 6), ("pad", "u1", 2),
                 ("laddr", "u1", 16), ("raddr", "u1", 16)])
DST = np.dtype([("addr", "u1", 16), ("dmac", "u1", 6), ("port", "<u2")])
DESC = np.dtype([("data_len", "<u2"), ("ip_id", "<u2"), ("sock", "u1"), ("tos", "u1"),
                 ("dst", "<u2")])


def _le16(v: int) -> bytes:  # a field "as stored": the native word's bytes
    return bytes((v & 0xFF, v >> 8))


def _be16(v: int) -> bytes:
    return bytes((v >> 8, v & 0xFF))


def hdr_len(af: int) -> int:
    return 14 + (20 if af == 4 else 40) + 8


def status_of(desc, socks, ndst: int, slot_bytes: int, zero_udp: bool) -> int:
    s = int(desc["sock"])
    if s >= len(socks) or int(socks[s]["af"]) not in (4, 6):
        return MALFORMED
    sk = socks[s]
    if not int(sk["flags"]) & SOCK_CONNECTED and int(desc["dst"]) >= ndst:
        return MALFORMED
    flen = hdr_len(int(sk["af"])) + int(desc["data_len"])
    if flen > 65535:
        return MALFORMED
    if flen > slot_bytes:
        return TRUNCATED
    return SEALED_ZERO_UDP if zero_udp else SEALED


def build_frame(desc, socks, dsts, payload: bytes, zero_udp: bool = False):
    """(frame bytes, ip header checksum, udp checksum) of a descriptor that
    passes the checks; `payload` is the data_len bytes behind the headers."""
    sk = socks[int(desc["sock"])]
    af, fl = int(sk["af"]), int(sk["flags"])
    dl, tos = int(desc["data_len"]), int(desc["tos"])
    assert len(payload) == dl
    conn = bool(fl & SOCK_CONNECTED)
    dst = None if conn else dsts[int(desc["dst"])]
    na = 4 if af == 4 else 16
    dmac = bytes(sk["dmac"]) if conn else bytes(dst["dmac"])
    raddr = bytes(sk["raddr"][:na]) if conn else bytes(dst["addr"][:na])
    dport = int(sk["rport"]) if conn else int(dst["port"])
    eth = dmac + bytes(sk["smac"]) + (b"\x08\x00" if af == 4 else b"\x86\xdd")
    ecn_default = (tos & 3) == 0 and bool(fl & SOCK_ECN)
    if af == 4:
        ip = bytearray(bytes((0x45, tos | (2 if ecn_default else 0))) + _be16(28 + dl) +
                       _le16(int(desc["ip_id"])) + b"\x40\x00" + b"\xff\x11" + b"\x00\x00" +
                       bytes(sk["laddr"][:4]) + raddr)
    else:
        if tos & 3:
            w = bytes((0x60 | (tos >> 4), (tos & 0x0F) << 4, 0, 0))
        else:
            w = bytes((0x60, 0, 0x20 if ecn_default else 0, 0))
        ip = bytearray(w + _be16(8 + dl) + b"\x11\xff" + bytes(sk["laddr"]) + raddr)
    hl = len(ip)
    udp = _le16(int(sk["lport"])) + _le16(dport) + _be16(8 + dl) + b"\x00\x00"
    pkt = ip + udp + payload
    ipck = udpck = 0
    if af == 4:
        ipck = c_oracle.ip_cksum(bytes(pkt[:20]))
        pkt[10:12] = _le16(ipck)
    if not zero_udp:
        zeroed = bytearray(pkt)
        udpck = c_oracle.payload_cksum(bytes(zeroed), hl + 8 + dl)
        pkt[hl + 6:hl + 8] = _le16(udpck)
    return eth + bytes(pkt), ipck, udpck


class Expect:
    """A batch's expectation: the whole buffer after the build, frame lengths,
    status codes, both value arrays and the error count."""

    def __init__(self, buf: np.ndarray, offs, descs, socks, dsts, slot_bytes: int,
                 zero_udp: bool = False):
        self.buf = buf.copy()
        n = len(offs)
        self.status = np.empty(n, np.uint8)
        self.frame_len = np.zeros(n, np.uint16)
        self.ip_hdr = np.zeros(n, np.uint16)
        self.udp = np.zeros(n, np.uint16)
        for i in range(n):
            d, o = descs[i], int(offs[i])
            st = status_of(d, socks, len(dsts), slot_bytes, zero_udp)
            self.status[i] = st
            if st > SEALED_ZERO_UDP:
                continue
            hb = hdr_len(int(socks[int(d["sock"])]["af"]))
            dl = int(d["data_len"])
            payload = b"" if zero_udp else buf[o + hb:o + hb + dl].tobytes()
            if zero_udp:  # (no payload byte is read: none is needed)
                fr, ipck, udpck = build_frame(d, socks, dsts, bytes(dl), True)
            else:
                fr, ipck, udpck = build_frame(d, socks, dsts, payload, False)
            self.buf[o:o + hb] = np.frombuffer(fr[:hb], np.uint8)
            self.frame_len[i] = hb + dl
            self.ip_hdr[i], self.udp[i] = ipck, udpck
        self.errors = int((self.status > SEALED_ZERO_UDP).sum())
