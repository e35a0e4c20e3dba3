"""Inputs shared by the tests that pin this project to the reference's own
checksum object (oracle/ref_oracle.py): the case generators of
tests/test_reference.py and tests/golden/make_ref_vectors.py, and the parts
of tests/golden/ref_vectors.npz that are rebuilt, not stored (the strided
packets' bodies, the Ethernet frames around the `fu` packets).

Every payload_cksum case has len >= header length by construction: below it
the reference has no behaviour (it reads ~4 GiB past the buffer).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from packets import ipv4_udp, ipv6_udp, pack

GOLDEN = Path(__file__).resolve().parent / "golden"
REF_VECTORS = GOLDEN / "ref_vectors.npz"

IP_STARTS = range(16)
IP_LENS = list(range(0, 131)) + [255, 256, 257, 511, 1471, 1472, 1473, 9000, 9001, 65534, 65535]
# the fixture's subset (the issue's list for it: no 511, no 65534)
IP_LENS_FIXTURE = list(range(0, 131)) + [255, 256, 257, 1471, 1472, 1473, 9000, 9001, 65535]


def hdr_len(first_byte):
    """4 * IHL where the high nibble is 4, else 40 (scalar or array)."""
    b = np.asarray(first_byte).astype(np.int64)
    return np.where(b >> 4 == 4, (b & 0x0F) * 4, 40)


def ip_sweep(lengths=IP_LENS):
    """(offs, lens): every start phase 0..15 x every length."""
    offs = [s for s in IP_STARTS for _ in lengths]
    lens = [ln for _ in IP_STARTS for ln in lengths]
    return np.array(offs, np.uint64), np.array(lens, np.uint16)


def redraw_lens(buf, offs, lens, rng):
    """len redrawn uniformly in [hl, len] for every packet."""
    hl = hdr_len(buf[offs.astype(np.int64)])
    ln = lens.astype(np.int64)
    assert (ln >= hl).all()
    return (hl + (rng.random(ln.size) * (ln - hl + 1)).astype(np.int64)).astype(np.uint16)


def ipv6_wrap_packets(rng):
    """The next_hdr << 24 uint32 wrap: all-0xFF jumbo payloads x next_hdr."""
    return [ipv6_udp(bytes([0xFF]) * p, rng, next_hdr=nh)
            for p in (60000, 65000, 65487) for nh in (17, 58, 128, 200, 255)]


def ipv4_totlen_wrap_packets(rng):
    """IPv4 with total length < hl, every value, every IHL 5..15: the 16-bit
    pseudo-header length bswap16(bswap16(ip->len) - hl) wraps."""
    pkts = []
    for ihl in range(5, 16):
        for tot in range(0, ihl * 4):
            pkt, ln = ipv4_udp(rng.integers(0, 256, int(rng.integers(0, 64)),
                                            dtype=np.uint8).tobytes(), rng, ihl=ihl)
            b = bytearray(pkt)
            b[2:4] = bytes([tot >> 8, tot & 0xFF])
            pkts.append((bytes(b), ln))
    return pkts


def nibble_grid_packets(rng, bodies=(0, None)):
    """Every version nibble x every IHL nibble: 40 random header bytes under
    that first byte, then a body; len = hl + body (body None: 1..63 random),
    so len == hl (no body at all) is there for each first byte."""
    pkts = []
    for first in range(256):
        hl = int(hdr_len(first))
        for body in bodies:
            body = int(rng.integers(1, 64)) if body is None else body
            b = bytearray(rng.integers(0, 256, max(hl + body, 40), dtype=np.uint8).tobytes())
            b[0] = first
            pkts.append((bytes(b), hl + body))
    return pkts


def random_byte_cases(rng, count, max_body=2000):
    """Pure random bytes with a random first byte, len = hl + U[0, max_body),
    packed back to back, and one case more at len 65535.
    -> (buf, offs, lens)"""
    first = rng.integers(0, 256, count + 1).astype(np.uint8)
    hl = hdr_len(first)
    lens = hl + rng.integers(0, max_body, count + 1)
    lens[-1] = 65535
    span = np.maximum(lens, 40)
    offs = np.concatenate(([0], np.cumsum(span)[:-1])) + 3
    buf = rng.integers(0, 256, int(offs[-1] + span[-1]) + 64, dtype=np.uint8)
    buf[offs] = first
    return buf, offs.astype(np.uint64), lens.astype(np.uint16)


# ---------------------------------------------------------------------------
# tests/golden/ref_vectors.npz: what is rebuilt at load.

ST_SHAPES = ((20, 20), (64, 64), (1472, 1472), (1500, 2048))  # (length, stride)
ST_N = 256
ST_HDR = 68  # stored bytes per strided packet: the longest IPv4 header + UDP's


def st_headers(rng, length):
    """(ST_N, min(ST_HDR, length)) header bytes of strided packets of `length`
    bytes: IPv4 + UDP, IPv6 + UDP where 48 bytes fit (a few with next_hdr 254 /
    255), IPv4 options where they fit; at length 20 the bare IPv4 header
    (len == hl)."""
    w = min(ST_HDR, length)
    out = np.zeros((ST_N, w), np.uint8)
    for i in range(ST_N):
        if length < 28:
            pkt = bytearray(ipv4_udp(b"", rng)[0][:20])
            pkt[2:4] = bytes([0, 20])
        elif i % 2 and length >= 48:
            # every fourth IPv6 header: next_hdr 255 / 254, whose << 24 wraps
            # the uint32 over a random MTU-size body (255) or just does not
            nh = {1: 255, 5: 254}.get(i % 8, 17)
            pkt = ipv6_udp(bytes(length - 48), rng, next_hdr=nh)[0]
        else:
            ihl = 5 if i % 4 else int(rng.integers(5, min(15, (length - 8) // 4) + 1))
            pkt = ipv4_udp(bytes(length - 8 - 4 * ihl), rng, ihl=ihl)[0]
        assert len(pkt) == length
        out[i] = np.frombuffer(bytes(pkt[:w]), np.uint8)
    return out


def st_blob(g, k: int) -> np.ndarray:
    """Strided group k of the fixture: the project's counter-based byte stream
    (oracle synth, the same bytes as wc_synth_fill) under the stored headers,
    packet i at i * stride; 64 spare bytes at the end."""
    from oracle import c_oracle
    length, stride = ST_SHAPES[k]
    hdr = g[f"st{k}_hdr"]
    blob = c_oracle.synth(ST_N * stride + 64, int(g["st_seed"]) + k)
    blob[: ST_N * stride].reshape(ST_N, stride)[:, : hdr.shape[1]] = hdr
    return blob


def tx_frames(g):
    """Ethernet frames around the fixture's `fu` packets, packed at odd
    addresses, both checksum fields overwritten (0x0000 / 0xFFFF / a pattern)
    -> (buf, offs, frame lens)."""
    blob = g["pl_blob"]
    frames = []
    for i, (o, ln) in enumerate(zip(g["fu_off"].tolist(), g["fu_len"].tolist())):
        pkt = bytearray(blob[o:o + ln].tobytes())
        v4 = pkt[0] >> 4 == 4
        hl = (pkt[0] & 0x0F) * 4 if v4 else 40
        fill = (0x0000, 0xFFFF, (i * 0x9E37 + 0x1234) & 0xFFFF)[i % 3].to_bytes(2, "little")
        if v4:
            pkt[10:12] = fill
        pkt[hl + 6:hl + 8] = fill
        mac = bytes((i * 7 + k * 13) & 0xFF for k in range(12))
        fr = mac + (b"\x08\x00" if v4 else b"\x86\xdd") + bytes(pkt)
        frames.append((fr, len(fr)))
    return pack(frames, align=1, lead=5)


def hdr_expect(blob, offs):
    """ip_cksum(ip, hl) of each IPv4 packet by the reference; 0 for IPv6."""
    from oracle import ref_oracle
    first = blob[offs.astype(np.int64)]
    v4 = first >> 4 == 4
    hl = np.where(v4, (first & 0x0F).astype(np.uint16) * 4, 0).astype(np.uint16)
    return np.where(v4, ref_oracle.cksum_ragged(blob, offs, hl, kind=0), 0).astype(np.uint16)


def expects(g) -> dict:
    """Every *_expect of the fixture `g` (a mapping with its inputs), computed
    by the live reference object."""
    import tx_model
    from oracle import ref_oracle
    out = {"ip_expect": ref_oracle.cksum_ragged(g["ip_blob"], g["ip_off"], g["ip_len"], kind=0),
           "pl_expect": ref_oracle.cksum_ragged(g["pl_blob"], g["pl_off"], g["pl_len"], kind=1),
           "fu_hdr_expect": hdr_expect(g["pl_blob"], g["fu_off"]),
           "fu_pl_expect": ref_oracle.cksum_ragged(g["pl_blob"], g["fu_off"], g["fu_len"], kind=1)}
    for k, (length, stride) in enumerate(ST_SHAPES):
        blob = st_blob(g, k)
        offs = np.arange(ST_N, dtype=np.uint64) * stride
        lens = np.full(ST_N, length, np.uint16)
        out[f"st{k}_ip_expect"] = ref_oracle.cksum_ragged(blob, offs, lens, kind=0)
        out[f"st{k}_pl_expect"] = ref_oracle.cksum_ragged(blob, offs, lens, kind=1)
        out[f"st{k}_hdr_expect"] = hdr_expect(blob, offs)
    buf, offs, lens = tx_frames(g)
    saved = tx_model.c_oracle
    tx_model.c_oracle = ref_oracle  # the model's two checksum calls, by the reference
    try:
        e = tx_model.Expect(buf, offs, lens)
    finally:
        tx_model.c_oracle = saved
    out.update(tx_status=e.status, tx_hdr_expect=e.ip_hdr, tx_udp_expect=e.udp)
    return out
