"""CPU tests of RX delivery: the tests' model of struct wc_rx_record
(tests/rx_deliver_model.py, udp.c:101-142 line by line) on frames whose fields
are known by construction, and the argument checks of the new C entry points,
which run before any device is touched."""
import ctypes
import struct

import numpy as np
import pytest

import rx_deliver_model as model
from oracle import c_oracle
from packets import RX_CASES, eth_frame, finish_udp, ipv4_udp, ipv6_udp, rx_frame
from warpcore_amd import _lib, cksum

OK, OK_NO_CKSUM = 0, 1


def frame4(rng, ihl=5, tos=0x2E, ttl=61, sport=0x1234, dport=0xABCD, plen=100, ulen=None,
           tot_delta=0, zero_udp=False):
    """An IPv4 / UDP Ethernet frame with every delivered field chosen here."""
    payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    pkt, _ = ipv4_udp(payload, rng, ihl=ihl, tot_len_delta=tot_delta)
    b = bytearray(pkt)
    hl = ihl * 4
    b[1], b[8] = tos, ttl
    b[hl:hl + 4] = struct.pack(">HH", sport, dport)
    if ulen is not None:
        b[hl + 4:hl + 6] = struct.pack(">H", ulen)
    return eth_frame(finish_udp(bytes(b), zero_udp=zero_udp), rng, 0x0800)


def frame6(rng, tclass=0xA5, hlim=33, sport=0x0102, dport=0xFEDC, plen=64):
    payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    pkt, _ = ipv6_udp(payload, rng)
    b = bytearray(pkt)
    b[0] = 0x60 | (tclass >> 4)
    b[1] = ((tclass & 0x0F) << 4) | (b[1] & 0x0F)
    b[7] = hlim
    b[40:44] = struct.pack(">HH", sport, dport)
    return eth_frame(finish_udp(bytes(b)), rng, 0x86DD)


def as_stored(port_be: int) -> int:
    """A network-order port as the little-endian host reads the field."""
    return ((port_be & 0xFF) << 8) | (port_be >> 8)


def rec(frame: bytes) -> dict:
    r = model.record_of(frame, len(frame))
    return {k: int(r[k]) for k in model.RECORD.names}


@pytest.mark.parametrize("ihl", [5, 6, 15])
def test_model_ipv4_header_lengths(ihl):
    rng = np.random.default_rng(ihl)
    fr = frame4(rng, ihl=ihl, plen=100)
    assert c_oracle.rx_verdict(fr) == OK
    hl = 4 * ihl
    assert rec(fr) == dict(data_off=14 + hl + 8, data_len=100, sport=as_stored(0x1234),
                           dport=as_stored(0xABCD), af=4, tos=0x2E, ttl=61, hl=hl,
                           src_off=26, dst_off=30)


def test_model_ipv6_traffic_class():
    """ip6_tos puts the class together from two nibbles of two bytes
    (ip6.h:77-81): 0xA5 checks that neither is dropped or swapped."""
    rng = np.random.default_rng(6)
    fr = frame6(rng, tclass=0xA5)
    assert c_oracle.rx_verdict(fr) == OK
    assert rec(fr) == dict(data_off=14 + 40 + 8, data_len=64, sport=as_stored(0x0102),
                           dport=as_stored(0xFEDC), af=6, tos=0xA5, ttl=33, hl=40,
                           src_off=22, dst_off=38)
    assert rec(frame6(rng, tclass=0x5A))["tos"] == 0x5A


def test_model_udp_len_against_ip_plen():
    """i->len = MIN(udp->len, ip_plen) - 8 (udp.c:128-129), either way round."""
    rng = np.random.default_rng(8)
    small = frame4(rng, plen=100, ulen=8 + 40)       # udp->len < ip_plen = 108
    assert c_oracle.rx_verdict(small) == OK and rec(small)["data_len"] == 40
    big = frame4(rng, plen=100, ulen=8 + 100 + 50)   # udp->len > ip_plen
    assert c_oracle.rx_verdict(big) == OK and rec(big)["data_len"] == 100


def test_model_zero_checksum_len_past_frame():
    """A zero-checksum datagram is accepted unverified (udp.c:132), so its
    udp->len is never held against the slot: the record says what the
    reference's i->len says, past the frame's end."""
    rng = np.random.default_rng(9)
    fr = frame4(rng, plen=100, ulen=8 + 400, tot_delta=500, zero_udp=True)
    assert c_oracle.rx_verdict(fr) == OK_NO_CKSUM
    r = rec(fr)
    assert r["data_len"] == 400 and r["data_off"] + r["data_len"] > len(fr)


def test_model_wire_layout():
    """The model's dtype is the C struct: 16 bytes, fields at the header's offsets."""
    rng = np.random.default_rng(10)
    fr = frame4(rng, ihl=7, plen=10)
    raw = model.record_of(fr, len(fr)).tobytes()
    assert len(raw) == 16 and model.RECORD == cksum.RX_RECORD
    assert struct.unpack("<HHHHBBBBHH", raw) == (14 + 28 + 8, 10, as_stored(0x1234),
                                                 as_stored(0xABCD), 4, 0x2E, 61, 28, 26, 30)


@pytest.mark.parametrize("case", RX_CASES)
def test_model_every_rx_case(case):
    """Zero unless the oracle accepts the frame; an accepted frame's record
    points at its own bytes."""
    rng = np.random.default_rng(RX_CASES.index(case) + 100)
    for _ in range(8):
        fr, flen = rx_frame(rng, case, max_payload=300)
        v = c_oracle.rx_verdict(fr, flen)
        r = model.record_of(fr, flen)
        if v not in (OK, OK_NO_CKSUM):
            assert r.tobytes() == bytes(16)
            continue
        v4 = fr[12:14] == b"\x08\x00"
        hl = (fr[14] & 15) * 4 if v4 else 40
        assert (int(r["af"]), int(r["hl"]), int(r["data_off"])) == (4 if v4 else 6, hl, 22 + hl)
        assert fr[14 + hl:14 + hl + 4] == struct.pack("<HH", int(r["sport"]), int(r["dport"]))
        assert int(r["data_off"]) <= flen and int(r["dst_off"]) + (4 if v4 else 16) <= flen


def test_model_select():
    v = np.array([0, 1, 7, 8, 3, 40, 255, 31, 0], np.uint8)
    assert model.select(v, model.MASK_DELIVER).tolist() == [0, 1, 8]
    assert model.select(v, model.MASK_HOST).tolist() == [2, 3]
    assert model.select(v, 0).size == 0
    assert model.select(v, 0xFFFFFFFF).tolist() == [0, 1, 2, 3, 4, 7, 8]
    assert (cksum.RX_MASK_DELIVER, cksum.RX_MASK_HOST) == (model.MASK_DELIVER, model.MASK_HOST)


def test_select_scratch_is_arithmetic():
    lib = _lib.load()
    assert lib.wc_rx_select_scratch(0) == 0
    prev = 0
    for n in [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 22) + 1, 1 << 32]:
        cur = lib.wc_rx_select_scratch(n)
        assert cur >= prev and cur > 0
        prev = cur
    assert cksum.rx_select_scratch(1 << 21) == lib.wc_rx_select_scratch(1 << 21)


def test_deliver_argument_errors_need_no_gpu():
    """Every check below returns before a device is touched."""
    lib = _lib.load()
    ok, einval = 0, -10001
    p = 0x100000  # 16-byte aligned, never dereferenced
    big = (1 << 32) + 1
    # empty batches (no count pointer: nothing to write)
    assert lib.wc_rx_select(None, 0, 3, None, None, None, None) == ok
    assert lib.wc_rx_deliver_ragged(None, None, None, 0, None, None, None, None, None, None,
                                    None) == ok
    # more frames than a uint32 index can name
    assert lib.wc_rx_select(p, big, 3, p, p, p, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, big, p, p, p, p, None, p, None) == einval
    # wc_rx_select: every pointer is needed
    assert lib.wc_rx_select(None, 8, 3, p, p, p, None) == einval
    assert lib.wc_rx_select(p, 8, 3, None, p, p, None) == einval
    assert lib.wc_rx_select(p, 8, 3, p, None, p, None) == einval
    assert lib.wc_rx_select(p, 8, 3, p, p, None, None) == einval
    # wc_rx_deliver_ragged: frames, verdicts and records; list and count together;
    # scratch with a list; records 16-byte aligned
    assert lib.wc_rx_deliver_ragged(None, p, p, 8, p, p, None, None, None, None, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, None, 8, p, p, None, None, None, None, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, None, p, None, None, None, None, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, p, None, None, None, None, None, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, p, p + 8, None, None, None, None, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, p, p, p, None, None, p, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, p, p, None, p, None, p, None) == einval
    assert lib.wc_rx_deliver_ragged(p, p, p, 8, p, p, p, p, None, None, None) == einval


def test_deliver_host_wrapper_empty_batch_needs_no_gpu():
    """The Python wrapper on an empty ring: WC_OK and empty results (its list
    pointer is never NULL beside the count it passes)."""
    v, r, lst, drops = cksum.rx_deliver_host(np.zeros(64, np.uint8), np.zeros(0, np.uint64),
                                             np.zeros(0, np.uint16))
    assert (v.size, r.size, lst.size, drops) == (0, 0, 0, 0)


def test_deliver_host_argument_errors_need_no_gpu():
    lib = _lib.load()
    ok, einval = 0, -10001
    buf = np.zeros(100, dtype=np.uint8)
    off = np.array([50], dtype=np.uint64)
    ln = np.array([20], dtype=np.uint16)
    ver = np.zeros(1, dtype=np.uint8)
    recs = np.zeros(1, dtype=cksum.RX_RECORD)
    lst = np.zeros(1, dtype=np.uint32)
    b, o, n_, v, r, li = (a.ctypes.data for a in (buf, off, ln, ver, recs, lst))
    cnt, drops = ctypes.c_uint64(7), ctypes.c_uint64(7)
    # an empty batch writes both counts
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 0, None, None, None, ctypes.byref(cnt),
                                  ctypes.byref(drops)) == einval  # a count without a list
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 0, None, None, li, ctypes.byref(cnt),
                                  ctypes.byref(drops)) == ok
    assert (cnt.value, drops.value) == (0, 0)
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 0, None, None, None, None, None) == ok
    # missing result arrays; list without count; too many frames
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 1, None, r, None, None, None) == einval
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 1, v, None, None, None, None) == einval
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 1, v, r, li, None, None) == einval
    assert lib.wc_rx_deliver_host(b, 100, o, n_, (1 << 32) + 1, v, r, None, None, None) == einval
    # a frame past the region
    off[0] = 90
    assert lib.wc_rx_deliver_host(b, 100, o, n_, 1, v, r, None, None, None) == einval
    # NULL frames
    assert lib.wc_rx_deliver_host(None, 100, o, n_, 1, v, r, None, None, None) == einval
