"""What RX delivery must give for a frame, restated for the tests (wc_cksum.h,
struct wc_rx_record): the record follows udp_rx line by line (udp.c:101-142,
163-165) in pure Python; whether a frame has one at all is the C oracle's
verdict (c_oracle.rx_verdict: OK / OK_NO_CKSUM), never this file's own parse.
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle

OK, OK_NO_CKSUM, NOT_UDP, NOT_IP = 0, 1, 7, 8
MASK_DELIVER = (1 << OK) | (1 << OK_NO_CKSUM)
MASK_HOST = (1 << NOT_UDP) | (1 << NOT_IP)

# struct wc_rx_record, field by field (16 bytes, little-endian)
RECORD = np.dtype([("data_off", "<u2"), ("data_len", "<u2"), ("sport", "<u2"), ("dport", "<u2"),
                   ("af", "u1"), ("tos", "u1"), ("ttl", "u1"), ("hl", "u1"),
                   ("src_off", "<u2"), ("dst_off", "<u2")])
assert RECORD.itemsize == 16


def _native16(b: bytes, at: int) -> int:
    """A uint16 field as the (little-endian) host reads it, bytes unswapped."""
    return b[at] | (b[at + 1] << 8)


def _bswap16(v: int) -> int:
    return ((v & 0xFF) << 8) | (v >> 8)


def udp_rx_fields(frame: bytes) -> dict:
    """udp_rx on a frame it is handed (eth_rx and ip4_rx / ip6_rx have passed
    it on): the w_iov fields it fills, as record fields.  Only called for a
    frame the oracle accepts, so every byte read here is inside the frame."""
    ip = 14                                   # udp.c:94  eth_data(buf)
    v = frame[ip] >> 4                        # udp.c:95  ip_v(*ip)
    if v == 4:                                # udp.c:101
        hl = (frame[ip] & 0x0F) * 4           # udp.c:103 ip4_hl(ip4->vhl)
        ip_plen = (_bswap16(_native16(frame, ip + 2)) - hl) & 0xFFFF  # udp.c:104 (uint16)
        af = 4                                # udp.c:106 AF_INET
        src_off, dst_off = ip + 12, ip + 16   # udp.c:107-108 ip4->src, ip4->dst
        tos = frame[ip + 1]                   # udp.c:109 i->flags = ip4->tos
        ttl = frame[ip + 8]                   # udp.c:110 i->ttl = ip4->ttl
    else:
        hl = 40                               # udp.c:113 sizeof(*ip6)
        ip_plen = _bswap16(_native16(frame, ip + 4))  # udp.c:114
        af = 6                                # udp.c:116 AF_INET6
        src_off, dst_off = ip + 8, ip + 24    # udp.c:117-118 ip6->src, ip6->dst
        vtcecnfl = int.from_bytes(frame[ip:ip + 4], "little")
        tos = (((vtcecnfl & 0x0000F000) >> 12) | ((vtcecnfl & 0x0000000F) << 4)) & 0xFF  # ip6.h:77-81
        ttl = frame[ip + 7]                   # udp.c:120 ip6->hlim
    udp = ip + hl                             # udp.c:105 / 115
    udp_len = min(_bswap16(_native16(frame, udp + 4)), ip_plen)  # udp.c:128
    data_len = (udp_len - 8) & 0xFFFF         # udp.c:129 i->len (uint16_t)
    sport = _native16(frame, udp)             # udp.c:141 udp->sport, as stored
    dport = _native16(frame, udp + 2)         # udp.c:142 udp->dport, as stored
    data_off = udp + 8                        # udp.c:165 i->buf
    return dict(data_off=data_off, data_len=data_len, sport=sport, dport=dport, af=af, tos=tos,
                ttl=ttl, hl=hl, src_off=src_off, dst_off=dst_off)


def record_of(frame: bytes, flen: int, verdict=None) -> np.ndarray:
    """One frame's struct wc_rx_record (a 0-d RECORD array): udp_rx's fields if
    the oracle's verdict is OK / OK_NO_CKSUM, sixteen zero bytes otherwise."""
    f = bytes(frame)[:flen]
    if verdict is None:
        verdict = c_oracle.rx_verdict(f, flen)
    r = np.zeros((), dtype=RECORD)
    if verdict in (OK, OK_NO_CKSUM):
        for k, val in udp_rx_fields(f).items():
            r[k] = val
    return r


def select(verdicts: np.ndarray, mask: int) -> np.ndarray:
    """wc_rx_select on the host: ascending indices whose code's bit is in mask."""
    v = np.asarray(verdicts, dtype=np.uint8)
    hit = (v < 32) & (((np.uint64(mask) >> np.minimum(v, 31).astype(np.uint64)) & np.uint64(1)) != 0)
    return np.flatnonzero(hit).astype(np.uint32)


class Expect:
    """A batch's expectation: the oracle's verdicts and drop count, the model's
    records, and the delivered-frame list (flatnonzero over the verdicts)."""

    def __init__(self, buf: np.ndarray, offs, lens):
        self.verdicts = c_oracle.rx_verdict_ragged(buf, offs, lens)
        n = len(offs)
        self.records = np.zeros(n, dtype=RECORD)
        for i in np.flatnonzero(np.isin(self.verdicts, (OK, OK_NO_CKSUM))).tolist():
            o, flen = int(offs[i]), int(lens[i])
            self.records[i] = record_of(buf[o:o + flen].tobytes(), flen, int(self.verdicts[i]))
        self.list = np.flatnonzero(np.isin(self.verdicts, (OK, OK_NO_CKSUM))).astype(np.uint32)
        self.drops = int(np.isin(self.verdicts, (2, 3, 4, 5, 6, 9)).sum())

    def take(self, idx) -> "Expect":
        """The expectation of the batch whose frame i is this one's frame
        idx[i] (a frame's verdict and record depend on its bytes alone)."""
        e = object.__new__(Expect)
        e.verdicts, e.records = self.verdicts[idx], self.records[idx]
        e.list = np.flatnonzero(np.isin(e.verdicts, (OK, OK_NO_CKSUM))).astype(np.uint32)
        e.drops = int(np.isin(e.verdicts, (2, 3, 4, 5, 6, 9)).sum())
        return e
