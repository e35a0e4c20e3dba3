"""Engine tables, frames and layouts for the RX reply tests: echo requests
(IPv4 and IPv6, valid and broken checksums) and other ICMP types, frames of
other IPv4 protocols, UDP frames for bound and unbound ports, ARP, and what
the filters turn away -- in scrambled 2048-byte slots or packed at every
16-byte phase."""
from __future__ import annotations

import numpy as np

import rx_reply_model as model
from oracle import c_oracle

MAC, PEER_MAC = bytes((2, 0, 0, 0, 0, 1)), bytes((2, 0, 0, 0, 0, 9))
A4 = [bytes((10, 1, 0, 1)), bytes((10, 1, 0, 2))]
BC4 = bytes((10, 1, 0, 255))
A6 = [bytes.fromhex("fe80000000000000020000fffe000001"),
      bytes.fromhex("20010db8000000000000000000000001")]
SNMA6 = [bytes.fromhex("ff0200000000000000000001ff000001")] * 2
BC6 = bytes.fromhex("ff020000000000000000000000000001")
PEER4, PEER6 = bytes((192, 168, 7, 7)), bytes.fromhex("20010db8000000000000000000000099")
PORT = 4433  # the one bound port of the worlds (both families)
# The worlds of the GPU tests, one per layout: (seed, frames, slot_bytes) -- the
# slots short enough that some echo finds no room.
WORLDS = {"slots": (101, 600, 256), "packed": (202, 600, 256)}


def engine_table(mtu: int = 1500, v6: int = 2, v4: int = 2, mac: bytes = MAC, rng=None):
    """Ours: v6 IPv6 entries first, then v4 IPv4 ones (ifaddr.c:94-146)."""
    addrs = [(6, A6[k], BC6, SNMA6[k]) for k in range(v6)]
    addrs += [(4, A4[k], BC4, None) for k in range(v4)]
    return model.engine(mac, mtu, addrs, rng)


def peer_table(mtu: int = 9000):
    """The other end's: every address a request of these cases comes from."""
    addrs = [(6, PEER6, BC6, SNMA6[0])] + [(6, a, BC6, SNMA6[0]) for a in A6]
    addrs += [(4, PEER4, BC4, None)] + [(4, a, BC4, None) for a in A4]
    return model.engine(PEER_MAC, mtu, addrs)


def _le16(v: int) -> bytes:
    return bytes((v & 0xFF, v >> 8))


def eth(body: bytes, etype: int, dst: bytes = MAC, src: bytes = PEER_MAC) -> bytes:
    return dst + src + etype.to_bytes(2, "big") + body


def ip4(payload: bytes, proto: int, src: bytes = PEER4, dst: bytes = None, ihl: int = 5,
        tot: int = None, rng=None) -> bytes:
    """An IPv4 packet with a valid header checksum; tot: ip->len as sent."""
    dst = A4[0] if dst is None else dst
    hl = 4 * ihl
    tot = hl + len(payload) if tot is None else tot
    opts = bytes(hl - 20) if rng is None else rng.integers(0, 256, hl - 20, dtype=np.uint8).tobytes()
    h = (bytes((0x40 | ihl, 0)) + (tot & 0xFFFF).to_bytes(2, "big") + b"\x12\x34\x40\x00" +
         bytes((64, proto)) + b"\x00\x00" + src + dst + opts)
    return h[:10] + _le16(c_oracle.ip_cksum(h)) + h[12:] + payload


def ip6(payload: bytes, nh: int, src: bytes = PEER6, dst: bytes = None, plen: int = None) -> bytes:
    dst = A6[0] if dst is None else dst
    plen = len(payload) if plen is None else plen
    return b"\x60\x00\x00\x00" + (plen & 0xFFFF).to_bytes(2, "big") + bytes((nh, 64)) + src + dst + payload


def icmp4_msg(typ: int, data: bytes, code: int = 0, rest: bytes = b"\xab\xcd\x00\x07") -> bytes:
    m = bytes((typ, code, 0, 0)) + rest + data
    return m[:2] + _le16(c_oracle.ip_cksum(m)) + m[4:]


def icmp6_pkt(typ: int, data: bytes, src: bytes = PEER6, dst: bytes = None, code: int = 0,
              rest: bytes = b"\xab\xcd\x00\x07") -> bytes:
    """An IPv6 packet carrying an ICMPv6 message with a valid checksum."""
    p = ip6(bytes((typ, code, 0, 0)) + rest + data, 58, src, dst)
    ck = c_oracle.payload_cksum(p, len(p))
    return p[:42] + _le16(ck) + p[44:]


def udp_pkt(af: int, data: bytes, dport: int, src: bytes = None, dst: bytes = None,
            zero: bool = False) -> bytes:
    u = (40000).to_bytes(2, "big") + dport.to_bytes(2, "big") + (8 + len(data)).to_bytes(2, "big") + \
        b"\x00\x00" + data
    if af == 4:
        p, hl = ip4(u, 17, PEER4 if src is None else src, dst), 20
    else:
        p, hl = ip6(u, 17, PEER6 if src is None else src, dst), 40
    if not zero:
        ck = c_oracle.payload_cksum(p, len(p))
        p = p[:hl + 6] + _le16(ck) + p[hl + 8:]
    return p


def echo4(data: bytes, ihl: int = 5, typ: int = 8, **kw) -> bytes:
    return eth(ip4(icmp4_msg(typ, data), 1, ihl=ihl, **kw), 0x0800)


def echo6(data: bytes, typ: int = 128, **kw) -> bytes:
    return eth(icmp6_pkt(typ, data, **kw), 0x86DD)


def flip(fr: bytes, at: int) -> bytes:
    b = bytearray(fr)
    b[at] ^= 0x40
    return bytes(b)


def world(seed: int, n: int, echo_max: int = 300):
    """n frames of every kind in a seeded mix: [(bytes, expected socket id or
    None where the frame is not delivered)].  Socket 0 / 1 are bound to
    (A4[0], PORT) / (A6[0], PORT)."""
    rng = np.random.default_rng(seed)
    out = []

    def data(most=echo_max):
        return rng.integers(0, 256, int(rng.integers(0, most + 1)), dtype=np.uint8).tobytes()

    kinds = 24
    for i in range(n):
        k = int(rng.integers(0, kinds)) if i >= kinds else i
        sk = None
        if k == 0:
            fr = echo4(data())
        elif k == 1:
            fr = echo6(data())
        elif k == 2:
            fr = echo4(data(), ihl=int(rng.integers(6, 16)), rng=rng)
        elif k == 3:  # a broken ICMP checksum, either family
            fr = echo4(data(40) + b"x")
            fr = flip(fr, int(rng.integers(34, len(fr))))
        elif k == 4:
            fr = echo6(data(40) + b"x")
            fr = flip(fr, int(rng.integers(54, len(fr))))
        elif k == 5:  # other ICMP types: only logged
            fr = echo4(data(60), typ=int(rng.choice([0, 3, 11, 13])))
        elif k == 6:
            fr = echo6(data(60), typ=int(rng.choice([129, 1, 133, 134])))
        elif k == 7:  # neighbour discovery: the host's
            fr = echo6(A6[0] + b"\x01\x01" + PEER_MAC, typ=int(rng.choice([135, 136])), dst=SNMA6[0])
            fr = b"\x33\x33\xff\x00\x00\x01" + fr[6:]
        elif k == 8:  # another IPv4 protocol (a TCP scan)
            fr = eth(ip4(data(80) + bytes(8), 6, ihl=int(rng.choice([5, 5, 7]))), 0x0800)
        elif k == 9:  # another IPv6 next header
            fr = eth(ip6(data(80), 6), 0x86DD)
        elif k in (10, 11):  # UDP to the bound port
            af = 4 if k == 10 else 6
            fr, sk = eth(udp_pkt(af, data(100), PORT), 0x0800 if af == 4 else 0x86DD), k - 10
        elif k in (12, 13):  # UDP to an unbound port from one of our own addresses: unreachable
            af = 4 if k == 12 else 6
            src = A4[1] if af == 4 else A6[1]
            fr = eth(udp_pkt(af, data(100) + bytes(40), 9, src=src, zero=bool(rng.integers(0, 2))),
                     0x0800 if af == 4 else 0x86DD)
            sk = model.SOCK_UNBOUND
        elif k in (14, 15):  # ... from a foreign address: nothing
            af = 4 if k == 14 else 6
            fr, sk = eth(udp_pkt(af, data(100), 9), 0x0800 if af == 4 else 0x86DD), model.SOCK_UNBOUND
        elif k == 16:  # an unbound IPv6 frame too short for the 48 copied bytes
            fr, sk = eth(udp_pkt(6, data(30), 9, src=A6[0]), 0x86DD), model.SOCK_UNBOUND
        elif k == 17:
            fr = eth(rng.integers(0, 256, 28, dtype=np.uint8).tobytes(), 0x0806, dst=b"\xff" * 6)
        elif k == 18:  # not our MAC
            fr = echo4(data(40))
            fr = bytes((2, 0, 0, 0, 0, int(rng.integers(2, 9)))) + fr[6:]
        elif k == 19:  # not our address
            fr = echo4(data(40), dst=bytes((10, 1, 0, int(rng.integers(3, 200)))))
        elif k == 20:
            fr = echo6(data(40), dst=PEER6)
        elif k == 21:  # broadcast echo
            fr = b"\xff" * 6 + echo4(data(40), dst=BC4 if rng.integers(0, 2) else b"\xff" * 4)[6:]
        elif k == 22:  # ip->len past the frame: the reference would copy its neighbour's bytes
            d = data(40)
            fr = eth(ip4(icmp4_msg(8, d), 1, tot=28 + len(d) + int(rng.integers(1, 9))), 0x0800)
        else:  # a drop of the RX verdict: a fragment
            b = bytearray(ip4(data(40) + bytes(8), 17))
            b[6:8] = b"\x00\x10"
            b[10:12] = b"\x00\x00"
            b[10:12] = _le16(c_oracle.ip_cksum(bytes(b[:20])))
            fr = eth(bytes(b), 0x0800)
        out.append((fr, sk))
    return out


def verdicts_of(frames):
    """The RX verdict of every frame, by the C oracle."""
    return np.array([c_oracle.rx_verdict(fr, len(fr)) for fr, _ in frames], np.uint8)


def socks_of(frames):
    """The socket ids rx_demux gives them: SOCK_NONE where not delivered."""
    return np.array([0xFE if sk is None else sk for _, sk in frames], np.uint8)


def slots(frames, rng, slot: int = 2048):
    """Scrambled `slot`-byte slots, each frame at a random byte phase inside
    its slot; random fill between the frames."""
    n = len(frames)
    idx = rng.permutation(n)
    buf = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
    offs = np.empty(n, np.uint64)
    for i, (fr, _) in enumerate(frames):
        o = int(idx[i]) * slot + int(rng.integers(0, min(16, slot - len(fr) + 1)))
        buf[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
        offs[i] = o
    return buf, offs, np.array([len(fr) for fr, _ in frames], np.uint16)


def packed(frames, rng, phase: int = 0):
    """Back to back from byte `phase` on, frame i + 1 at the next address that
    is (phase + i + 1) mod 16: every 16-byte phase occurs, gaps of 0..15 bytes."""
    offs = []
    buf = bytearray(rng.integers(0, 256, 16 + phase, dtype=np.uint8).tobytes())
    for i, (fr, _) in enumerate(frames):
        pad = (phase + i - len(buf)) % 16
        buf += rng.integers(0, 256, pad, dtype=np.uint8).tobytes()
        offs.append(len(buf))
        buf += fr
    buf += rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return (np.frombuffer(bytes(buf), np.uint8).copy(), np.array(offs, np.uint64),
            np.array([len(fr) for fr, _ in frames], np.uint16))


def out_slots(m: int, slot_bytes: int, rng, phased: bool = True):
    """m reply slots in a random-filled buffer with guard bytes around and
    between them: (buffer, offsets); slot j starts at phase j mod 16."""
    offs, pos = [], 32
    for j in range(m):
        pos += (j - pos) % 16 if phased else 0
        offs.append(pos)
        pos += slot_bytes + int(rng.integers(0, 9))
    buf = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    return buf, np.array(offs, np.uint64)


def _short_echo4(cut: int) -> bytes:
    """An IPv4 echo request of 8 ICMP bytes whose ip->len stops `cut` bytes
    early; the bytes cut off are zero, so the checksum holds either way."""
    return eth(ip4(icmp4_msg(8, b"", rest=b"\xab\xcd\x00\x00"), 1, tot=28 - cut), 0x0800)


def _echo6_plen(plen: int, msg_len: int = 8) -> bytes:
    """An IPv6 echo request of msg_len ICMPv6 bytes (zeros behind the id)
    whose ip6->len says plen, valid over the MIN(plen, msg_len) bytes
    icmp6_rx sums."""
    p = ip6((b"\x80\x00\x00\x00\xab\xcd" + bytes(msg_len))[:msg_len], 58, plen=plen)
    k = 40 + min(plen, msg_len)
    ck = c_oracle.payload_cksum(p[:k], k)
    return eth(p[:42] + _le16(ck) + p[44:], 0x86DD)


def _empty_icmp6() -> bytes:
    """next header 58, ip6->len 0, no byte behind the header, and a source
    address for which payload_cksum of the 40 bytes is 0."""
    p = bytearray(ip6(b"", 58))
    f = ~c_oracle.payload_cksum(bytes(p), 40) & 0xFFFF
    w = ((p[22] | (p[23] << 8)) - f) % 0xFFFF or 0xFFFF
    p[22:24] = _le16(w)
    assert c_oracle.payload_cksum(bytes(p), 40) == 0
    return eth(bytes(p), 0x86DD)


def grid():
    """One frame on each side of every comparison of the chain:
    [(name, frame, socket id or None, engine, slot_bytes, action, reply length)],
    the expectation stated by hand."""
    M = model
    E, U = engine_table(), M.SOCK_UNBOUND
    e100, no4 = engine_table(mtu=100), engine_table(v4=0)
    d58 = bytes(range(58))
    g = []

    def add(name, fr, act, ln=0, sock=None, eng=E, slot=2048):
        g.append((name, fr, sock, eng, slot, act, ln))

    # t against hl + 8, and the empty echo
    add("echo4 ip_len = hl + 8", _short_echo4(0), M.ECHO4, 42)
    add("echo4 ip_len = hl + 7", _short_echo4(1), M.MALFORMED)
    add("echo6 ip6_len = 8", _echo6_plen(8), M.ECHO6, 62)
    add("echo6 ip6_len = 7", _echo6_plen(7), M.MALFORMED)
    # 14 + t against flen
    add("echo4 ip_len = the frame's", echo4(d58), M.ECHO4, 100)
    add("echo4 ip_len one past the frame", eth(ip4(icmp4_msg(8, d58), 1, tot=87), 0x0800), M.MALFORMED)
    add("echo6 ip6_len = the frame's", _echo6_plen(66, 66), M.ECHO6, 120)
    add("echo6 ip6_len one past the frame", _echo6_plen(67, 66), M.MALFORMED)
    # ip_len against mtu
    add("echo4 ip_len = mtu", echo4(bytes(72)), M.ECHO4, 114, eng=e100)
    add("echo4 ip_len = mtu + 1", echo4(bytes(73)), M.ECHO4, 114, eng=e100)
    add("echo6 ip6_len = mtu - 40", echo6(bytes(52)), M.ECHO6, 114, eng=e100)
    add("echo6 ip6_len = mtu - 39", echo6(bytes(53)), M.ECHO6, 114, eng=e100)
    # the IPv4 header lengths
    for ihl in (6, 10, 15):
        add(f"echo4 ihl {ihl}", echo4(d58, ihl=ihl), M.ECHO4, 100)
        add(f"proto4 ihl {ihl}", eth(ip4(bytes(20), 6, ihl=ihl), 0x0800), M.UNREACH_PROTO4, 50 + 4 * ihl)
    # flen 101 / 102 for the IPv6 port unreachable
    u6 = lambda k: eth(udp_pkt(6, bytes(k), 9, src=A6[1]), 0x86DD)  # noqa: E731
    add("port6 flen 102", u6(40), M.UNREACH_PORT6, 110, sock=U)
    add("port6 flen 101", u6(39), M.MALFORMED, sock=U)
    # reply_len against slot_bytes
    add("slot = reply", echo4(d58), M.ECHO4, 100, slot=100)
    add("slot = reply - 1", echo4(d58), M.NO_ROOM, slot=99)
    add("port6 slot 109", u6(40), M.NO_ROOM, sock=U, slot=109)
    # the three MAC alternatives
    e4 = echo4(d58)
    add("mac broadcast", b"\xff" * 6 + e4[6:], M.ECHO4, 100)
    add("mac 33 33", b"\x33\x33\x01\x02\x03\x04" + e4[6:], M.ECHO4, 100)
    add("mac ff x 5", b"\xff" * 5 + b"\xfe" + e4[6:], M.FILTERED)
    add("mac 33 32", b"\x33\x32\x01\x02\x03\x04" + e4[6:], M.FILTERED)
    add("mac last byte", MAC[:5] + b"\x02" + e4[6:], M.FILTERED)
    add("arp, mac not ours", eth(bytes(28), 0x0806, dst=PEER_MAC), M.FILTERED)
    add("arp", eth(bytes(28), 0x0806, dst=b"\xff" * 6), M.HOST)
    # the address alternatives
    add("dst4 second address", echo4(d58, dst=A4[1]), M.ECHO4, 100)
    add("dst4 bcast", echo4(d58, dst=BC4), M.ECHO4, 100)
    add("dst4 255.255.255.255", echo4(d58, dst=b"\xff" * 4), M.ECHO4, 100)
    add("dst4 255.255.255.255, no af-4 entry", echo4(d58, dst=b"\xff" * 4), M.FILTERED, eng=no4)
    add("dst4 ours, no af-4 entry", echo4(d58), M.FILTERED, eng=no4)
    add("dst4 other", echo4(d58, dst=bytes((10, 1, 0, 3))), M.FILTERED)
    add("dst4 = an IPv6 entry's first bytes", echo4(d58, dst=A6[0][:4]), M.FILTERED)
    add("dst6 second address", echo6(d58, dst=A6[1]), M.ECHO6, 120)
    add("dst6 snma", echo6(d58, dst=SNMA6[0]), M.ECHO6, 120)
    add("dst6 bcast", echo6(d58, dst=BC6), M.ECHO6, 120)
    add("dst6 other", echo6(d58, dst=PEER6), M.FILTERED)
    add("dst6 = an IPv4 entry's bytes", echo6(d58, dst=A4[0] + bytes(12)), M.FILTERED)
    # source match against destination match for the unreachables
    u4 = lambda **kw: eth(udp_pkt(4, bytes(30), 9, **kw), 0x0800)  # noqa: E731
    add("port4 src ours", u4(src=A4[1]), M.UNREACH_PORT4, 70, sock=U)
    add("port4 src ours, zero checksum", u4(src=A4[0], zero=True), M.UNREACH_PORT4, 70, sock=U)
    add("port4 src foreign", u4(), M.NONE, sock=U)
    add("port4 src = bcast", u4(src=BC4), M.NONE, sock=U)
    add("port4 src ours, dst other", u4(src=A4[1], dst=bytes((10, 1, 0, 3))), M.FILTERED, sock=U)
    add("port4 bound", u4(src=A4[1]), M.NONE, sock=0)
    add("port4 no d_sock", u4(src=A4[1]), M.NONE)
    add("port6 src ours", u6(60), M.UNREACH_PORT6, 110, sock=U)
    add("port6 src foreign", eth(udp_pkt(6, bytes(60), 9), 0x86DD), M.NONE, sock=U)
    add("port6 src = snma", eth(udp_pkt(6, bytes(60), 9, src=SNMA6[0]), 0x86DD), M.NONE, sock=U)
    # the checksum verdicts and the types
    add("echo4 bad checksum", flip(e4, 50), M.ICMP_BAD_CKSUM)
    add("echo6 bad checksum", flip(echo6(d58), 70), M.ICMP_BAD_CKSUM)
    add("icmp4 no byte", eth(ip4(b"", 1), 0x0800), M.ICMP_BAD_CKSUM)
    add("icmp4 echo reply", echo4(d58, typ=0), M.NONE)
    add("icmp6 echo reply", echo6(d58, typ=129), M.NONE)
    add("icmp6 nsol", echo6(A6[0] + b"\x01\x01" + PEER_MAC, typ=135, dst=SNMA6[0]), M.HOST)
    add("icmp6 nadv", echo6(A6[0], typ=136), M.HOST)
    add("icmp6 nsol, bad checksum", flip(echo6(A6[0], typ=135), 60), M.ICMP_BAD_CKSUM)
    add("icmp6 no byte", _empty_icmp6(), M.MALFORMED)
    # the other protocols
    add("proto4 tcp", eth(ip4(bytes(20), 6), 0x0800), M.UNREACH_PROTO4, 70)
    add("proto4 8 bytes", eth(ip4(bytes(8), 6), 0x0800), M.UNREACH_PROTO4, 70)
    add("proto4 7 bytes", eth(ip4(bytes(7), 6), 0x0800), M.MALFORMED)
    add("ip6 tcp", eth(ip6(bytes(20), 6), 0x86DD), M.NONE)
    # a drop of the verdict in front
    frag = bytearray(ip4(bytes(20), 1))
    frag[6:8], frag[10:12] = b"\x00\x08", b"\x00\x00"
    frag[10:12] = _le16(c_oracle.ip_cksum(bytes(frag[:20])))
    add("fragment", eth(bytes(frag), 0x0800), M.NONE)
    return g
