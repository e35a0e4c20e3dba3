"""Worlds for the RX echo tests: a socket population (rx_demux_cases.population:
connected and bound sockets of both families), and a ring of frames built from
rx_demux_cases.udp_frame / frame_to -- both families, IHL 5 to 15, zero UDP
checksums, payloads of every length in LENS, strays that no socket takes -- with
frames that are not UDP in between (packets.rx_frame).  plan(): the records of
rx_deliver_model and the list / start of rx_demux_model, the inputs of
rx_echo_model.echo."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import rx_deliver_model as dmodel
import rx_demux_cases as dc
import rx_demux_model as xmodel
import rx_echo_model as model
import tx_build_model as bmodel
from packets import rx_frame

LENS = (0, 1, 2, 3, 15, 16, 17, 31, 33, 200, 1472)
NOT_UDP = ("icmp4", "icmp6", "arp")
MAC = bytes((2, 0, 0, 0, 0, 1))       # ours: the TX sockets' smac
PEERS4 = [bytes((192, 168, 7, k)) for k in (7, 8, 9)]
PEERS6 = [bytes(range(32, 47)) + bytes((k,)) for k in (1, 2, 3)]


class _Sized:
    """A generator whose next two-argument integers() draw is `length`:
    rx_demux_cases.udp_frame draws its payload length that way, first."""

    def __init__(self, rng, length: int):
        self._rng, self._length = rng, length

    def integers(self, *a, **kw):
        if self._length is not None and len(a) == 2 and not kw:
            v, self._length = self._length, None
            return v
        return self._rng.integers(*a, **kw)

    def __getattr__(self, name):
        return getattr(self._rng, name)


def sized_frame_to(rng, s, length: int, k: int = 0, **kw):
    """dc.frame_to with a payload of exactly `length` bytes; an unconnected
    socket hears from one of three peers of its family."""
    af = int(s["af"])
    peer = (PEERS4 if af == 4 else PEERS6)[k % 3]
    return dc.frame_to(_Sized(rng, length), s, remote=(peer, dc.be16(7000 + k % 5)), **kw)


def frames_of(rng, socks, n: int):
    """n frames: of every nine, one stray and one that is not UDP; the others
    go to the sockets in turn, their payload lengths walking LENS, every seventh
    IPv4 one with options (IHL 6 to 15), every fifth with a zero UDP checksum."""
    out, t = [], 0
    for k in range(n):
        if k % 9 == 4:
            out.append(dc.stray_frame(rng)[0])
        elif k % 9 == 8 or not len(socks):
            fr, flen = rx_frame(rng, NOT_UDP[(k // 9) % len(NOT_UDP)], 64)
            out.append(bytes(fr)[:flen])
        else:
            s = socks[t % len(socks)]
            ihl = 6 + (t // 7) % 10 if int(s["af"]) == 4 and t % 7 == 3 else 5
            out.append(sized_frame_to(rng, s, LENS[(t + t // len(LENS)) % len(LENS)], t, ihl=ihl,
                                      zero_udp=(t % 5 == 2))[0])
            t += 1
    return out


def tx_socks(socks) -> np.ndarray:
    """One unconnected TX socket per RX socket, on its local address and port."""
    out = np.zeros(len(socks), bmodel.SOCK)
    for t, s in zip(out, socks):
        t["af"], t["lport"] = s["af"], s["lport"]
        t["smac"] = np.frombuffer(MAC, np.uint8)
        t["laddr"] = s["laddr"]
        if int(s["af"]) == 4:
            t["laddr"][4:] = 0
    return out


def echo_map(ns: int, kind: str, one: int = 0) -> np.ndarray:
    """all / none / alternating (even sockets on) / single (socket `one`):
    socket s answers from TX socket s."""
    m = np.full(ns, model.OFF, np.uint16)
    on = {"all": range(ns), "none": (), "alternating": range(0, ns, 2),
          "single": (one,) if ns else ()}[kind]
    for s in on:
        m[s] = s
    return m


def plan(buf, offs, lens, socks):
    """What the drain leaves for the echo, from the models: records, the
    grouped list and start[256]; and each frame's socket id."""
    d = dmodel.Expect(buf, offs, lens)
    frames = [(buf[int(o):int(o) + int(ln)].tobytes(), int(ln)) for o, ln in zip(offs, lens)]
    x = xmodel.Expect(xmodel.Table(socks), frames, d.records)
    return SimpleNamespace(rec=d.records, list=x.list, start=x.start, sock=x.sock,
                           verdicts=d.verdicts)


def world(seed: int, n: int, ns: int):
    """(socks, frames) of one ring."""
    rng = np.random.default_rng(seed)
    socks = dc.population(ns, seed)
    return socks, frames_of(rng, socks, n)
