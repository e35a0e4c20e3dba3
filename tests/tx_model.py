"""What the TX seal must do to a frame, restated for the tests (wc_cksum.h,
enum wc_tx_status): the check chain in its order, the field reads modelled on
oracle/py_oracle.py:rx_verdict, the two values from the C oracle's ip_cksum /
payload_cksum on a copy of the frame with both fields zeroed.
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle

SEALED, SEALED_ZERO_UDP, IP_ONLY, NOT_UDP, NOT_IP, BAD_VERSION, MALFORMED, TRUNCATED = range(8)


class Seal:
    """One frame's expectation: status, the two values (0 where none is
    computed) and the stores as (frame offset, native uint16) pairs."""
    __slots__ = ("status", "ip_hdr", "udp", "stores", "hl", "udp_len")

    def __init__(self, status, ip_hdr=0, udp=0, stores=(), hl=0, udp_len=0):
        self.status, self.ip_hdr, self.udp, self.stores = status, ip_hdr, udp, tuple(stores)
        self.hl, self.udp_len = hl, udp_len


def seal_frame(frame: bytes, flen: int, zero_udp: bool = False) -> Seal:
    f = bytes(frame)[:flen]
    if flen < 14:
        return Seal(TRUNCATED)
    etype = (f[12] << 8) | f[13]
    if etype not in (0x0800, 0x86DD):
        return Seal(NOT_IP)
    ip = bytearray(f[14:])
    if not ip:
        return Seal(TRUNCATED)
    v4 = etype == 0x0800
    if ip[0] >> 4 != (4 if v4 else 6):
        return Seal(BAD_VERSION)
    ip_hdr, stores = 0, []
    if v4:
        hl = (ip[0] & 0x0F) * 4
        if hl < 20:
            return Seal(MALFORMED)
        if len(ip) < hl:
            return Seal(TRUNCATED)
        frag = (ip[6] | (ip[7] << 8)) & 0xFF1F  # IP4_OFFMASK on the native word
        proto = ip[9]
        ip_plen = (((ip[2] << 8) | ip[3]) - hl) & 0xFFFF
        ip[10:12] = b"\x00\x00"
        ip_hdr = c_oracle.ip_cksum(bytes(ip[:hl]))
        stores.append((14 + 10, ip_hdr))
    else:
        hl = 40
        if len(ip) < 40:
            return Seal(TRUNCATED)
        frag, proto = 0, ip[6]
        ip_plen = (ip[4] << 8) | ip[5]
    if proto != 17 or frag:
        return Seal(IP_ONLY, ip_hdr, 0, stores, hl) if v4 else Seal(NOT_UDP)
    if ip_plen < 8:
        return Seal(MALFORMED)
    if len(ip) < hl + 8:
        return Seal(TRUNCATED)
    udp_len = min((ip[hl + 4] << 8) | ip[hl + 5], ip_plen)
    if udp_len < 8:
        return Seal(MALFORMED)
    if zero_udp:
        stores.append((14 + hl + 6, 0))
        return Seal(SEALED_ZERO_UDP, ip_hdr, 0, stores, hl, udp_len)
    if len(ip) < hl + udp_len:
        return Seal(TRUNCATED)
    ip[hl + 6:hl + 8] = b"\x00\x00"
    udp = c_oracle.payload_cksum(bytes(ip), hl + udp_len)
    stores.append((14 + hl + 6, udp))
    return Seal(SEALED, ip_hdr, udp, stores, hl, udp_len)


def garble_fields(buf: np.ndarray, offs, lens, rng: np.random.Generator) -> None:
    """Overwrite both checksum fields of every IPv4 / IPv6 frame, where they
    lie inside it, with 0x00, 0xFF or random bytes: what they hold on entry
    must not matter."""
    for o, flen in zip(offs.tolist(), lens.tolist()):
        o = int(o)
        if flen < 15:
            continue
        etype = (int(buf[o + 12]) << 8) | int(buf[o + 13])
        if etype not in (0x0800, 0x86DD):
            continue
        hl = (int(buf[o + 14]) & 0x0F) * 4 if etype == 0x0800 else 40
        spots = ([14 + 10] if etype == 0x0800 else []) + [14 + hl + 6]
        for at in spots:
            if at + 2 > flen:
                continue
            k = int(rng.integers(0, 3))
            buf[o + at:o + at + 2] = (0x00, 0xFF)[k] if k < 2 else rng.integers(0, 256, 2)


class Expect:
    """A batch's expectation: the whole buffer after the seal, the status codes,
    both value arrays and the error count."""

    def __init__(self, buf: np.ndarray, offs, lens, zero_udp: bool = False):
        self.buf = buf.copy()
        n = len(offs)
        self.status = np.empty(n, np.uint8)
        self.ip_hdr = np.zeros(n, np.uint16)
        self.udp = np.zeros(n, np.uint16)
        self.seals = []
        for i, (o, flen) in enumerate(zip(offs.tolist(), lens.tolist())):
            o = int(o)
            s = seal_frame(buf[o:o + flen].tobytes(), flen, zero_udp)
            self.seals.append(s)
            self.status[i], self.ip_hdr[i], self.udp[i] = s.status, s.ip_hdr, s.udp
            for at, v in s.stores:
                self.buf[o + at] = v & 0xFF
                self.buf[o + at + 1] = v >> 8
        self.errors = int((self.status >= BAD_VERSION).sum())
