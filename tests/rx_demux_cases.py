"""Socket populations and frames for the RX demultiplex tests."""
from __future__ import annotations

import numpy as np

import rx_demux_model as model
from packets import eth_frame, finish_udp, ipv4_udp, ipv6_udp

A4 = [bytes([10, 1, 0, k]) for k in range(1, 9)]
A6 = [A4[0] + bytes([k] * 12) for k in range(1, 5)]  # A6[0] shares A4[0]'s four bytes
PEER4, PEER6 = bytes([192, 168, 7, 7]), bytes(range(32, 48))


def be16(port: int) -> int:
    """Port `port` as a little-endian host reads its network-order bytes."""
    return ((port & 0xFF) << 8) | (port >> 8)


def population(ns: int, seed: int) -> np.ndarray:
    """`ns` distinct sockets with every trap among them (from 17 sockets on;
    fewer hold as many as fit): a connected and a bound-only socket on one
    local pair, an IPv4 and an IPv6 socket alike in their first four address
    bytes and ports, one port on several addresses, sequential ports on one
    address -- and garbage in every ignored byte."""
    rng = np.random.default_rng(seed)
    out = [model.sock(4, A4[0], be16(4433), rng=rng),                         # 0 bound ...
           model.sock(4, A4[0], be16(4433), PEER4, be16(999), rng=rng),       # 1 ... and connected
           model.sock(6, A6[0], be16(4433), rng=rng),                         # 2 the v6 look-alike
           model.sock(6, A6[0], be16(4433), PEER6, be16(999), rng=rng),       # 3
           model.sock(4, A4[0], be16(4433), PEER4, be16(1000), rng=rng)]      # 4 another remote port
    out += [model.sock(4, a, be16(53), rng=rng) for a in A4[1:5]]              # one port, 4 addresses
    out += [model.sock(6, a, be16(53), rng=rng) for a in A6[1:4]]
    port = 5000
    while len(out) < ns:                                                      # sequential ports
        out.append(model.sock(4, A4[5], be16(port), rng=rng) if port % 3 else
                   model.sock(6, A6[1], be16(port), PEER6, be16(port + 1), rng=rng))
        port += 1
    return np.array(out[:ns], dtype=model.SOCK)


def udp_frame(rng, af: int, laddr: bytes, lport: int, raddr: bytes, rport: int,
              max_payload: int = 200, ihl: int = 5, zero_udp: bool = False):
    """An accepted UDP frame to local (laddr, lport) from remote (raddr,
    rport), ports as the header stores them read little-endian: (bytes, len)."""
    payload = rng.integers(0, 256, int(rng.integers(0, max_payload + 1)), dtype=np.uint8).tobytes()
    ports = int(rport).to_bytes(2, "little") + int(lport).to_bytes(2, "little")  # sport, dport
    if af == 4:
        b = bytearray(ipv4_udp(payload, rng, ihl=ihl)[0])
        b[12:16], b[16:20] = raddr, laddr
        b[ihl * 4:ihl * 4 + 4] = ports
    else:
        b = bytearray(ipv6_udp(payload, rng)[0])
        b[8:24], b[24:40] = raddr, laddr
        b[40:44] = ports
    fr = eth_frame(finish_udp(bytes(b), zero_udp=zero_udp), rng, 0x0800 if af == 4 else 0x86DD)
    return fr, len(fr)


def frame_to(rng, s, remote=None, **kw):
    """A frame for socket `s` (a SOCK entry): from its own remote if it is
    connected, else from `remote` = (addr, port) or a random one."""
    (af, la, lp), rem = model.sock_tuple(s)
    if rem is not None:
        ra, rp = rem[1], rem[2]
    elif remote is not None:
        ra, rp = remote
    else:
        ra, rp = rng.bytes(len(la)), int(rng.integers(1, 1 << 16))
    return udp_frame(rng, af, la, lp, ra, rp, **kw)


def stray_frame(rng, **kw):
    """An accepted UDP frame no population() socket takes."""
    af = 4 if rng.random() < 0.5 else 6
    alen = 4 if af == 4 else 16
    return udp_frame(rng, af, bytes([172]) + rng.bytes(alen - 1), int(rng.integers(1, 1 << 16)),
                     rng.bytes(alen), int(rng.integers(1, 1 << 16)), **kw)
