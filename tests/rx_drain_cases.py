"""Worlds for the RX drain tests: one ring that mixes, interleaved at random,
the frames of the three generators the chain's own tests use -- rx_demux_cases
(UDP frames for a socket population, strays), rx_reply_cases.world (ICMP echoes
of both families, broken ICMP sums, other protocols, foreign MAC / address,
unbound UDP from one of our own addresses) and rx_neigh_cases.world (ARP and
neighbour discovery of every CENSUS class) -- over rx_reply_cases' engine table
and a socket table on addresses that table holds, in rx_reply_cases' `slots`
and `packed` layouts (packed: every 16-byte phase, odd ones included).

expect() states every output of wc_rx_drain from the models alone: the C
oracle's verdicts, rx_deliver_model's records, wc_rx_socktab_lookup on the host
table, rx_demux_model.group, rx_reply_model.plan and rx_neigh_model.plan."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import rx_deliver_model as dmodel
import rx_demux_cases as dc
import rx_demux_model as xmodel
import rx_neigh_cases as nc
import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel
import warpcore_amd as wc

SMALL = 4096  # WC_RX_DRAIN_SMALL
# The worlds of the model test and of the GPU tests' 600-frame cases, one per
# layout: (seed, frames, sockets, slot_bytes) -- the slots short enough that
# some echo finds no room.
WORLDS = {"slots": (14, 600, 6, 256), "packed": (19, 600, 6, 256)}
# Of every 20 frames: 9 from rx_neigh_cases, 8 from rx_reply_cases, 3 from
# rx_demux_cases.  Some thirty-five classes share the 600 frames, so a class's
# count is near ten in most seeds: the worlds' seeds are ones at which every
# class of the three censuses occurs ten times (test_rx_drain_model.py).
SHARES = (9, 8, 3)


def sockets(ns: int, seed: int) -> np.ndarray:
    """`ns` distinct sockets: the bound port of rx_reply_cases' worlds in both
    families first (on the engine table's first addresses), then
    rx_demux_cases.population with its traps."""
    cand = [xmodel.sock(4, rc.A4[0], dc.be16(rc.PORT)), xmodel.sock(6, rc.A6[0], dc.be16(rc.PORT))]
    cand += list(dc.population(ns, seed))
    out, seen = [], set()
    for s in cand:
        t = xmodel.sock_tuple(s)
        if t not in seen:
            seen.add(t)
            out.append(s)
    return np.array(out[:ns], dtype=xmodel.SOCK)


def demux_frames(rng, socks, count: int):
    """`count` UDP frames: four of five for the sockets in turn (IPv4 options
    and zero checksums among them), every fifth a stray -- alternately one no
    socket could take and one to an unbound port of ours from one of our own
    addresses (udp_rx's port unreachable).  Two of three carry our MAC (the
    others rx_demux_cases' random one, which eth_rx turns away); every eleventh
    has its last byte flipped, so its UDP sum fails and its record is taken
    back."""
    out = []
    for k in range(count):
        if len(socks) and k % 5 != 4:
            s = socks[(k - k // 5) % len(socks)]
            fr = dc.frame_to(rng, s, ihl=5 + (k % 11 if k % 7 == 0 else 0),
                             zero_udp=(k % 13 == 0))[0]
        elif k % 10 == 4:
            fr = dc.stray_frame(rng)[0]
        else:
            a = rc.A4 if k % 20 == 9 else rc.A6
            fr = dc.udp_frame(rng, 4 if a is rc.A4 else 6, a[0], dc.be16(9000 + k), a[1],
                              dc.be16(40000), max_payload=120)[0]
        if k % 3:
            fr = rc.MAC + fr[6:]
        out.append(rc.flip(fr, len(fr) - 1) if k % 11 == 10 and k % 13 else fr)
    return out


def world(seed: int, n: int, ns: int):
    """(frames, socks): n frames of the three generators, shuffled, and the
    socket list they are demultiplexed by."""
    rng = np.random.default_rng(seed)
    socks = sockets(ns, seed)
    n_neigh, n_reply = n * SHARES[0] // 20, n * SHARES[1] // 20
    frames = [f[0] for f in nc.world(seed + 1, n_neigh)]
    frames += [f[0] for f in rc.world(seed + 2, n_reply)]
    frames += demux_frames(rng, socks, n - len(frames))
    return [frames[i] for i in rng.permutation(n)], socks


def layout(name: str, frames, seed: int):
    rng = np.random.default_rng(seed)
    pairs = [(fr, None) for fr in frames]
    return rc.slots(pairs, rng) if name == "slots" else rc.packed(pairs, rng, seed % 16)


def lookup(tab: np.ndarray, frame: bytes, rec) -> int:
    """wc_rx_socktab_lookup of a frame's record on the host table."""
    af = int(rec["af"])
    if af == 0:
        return xmodel.NONE
    alen = 4 if af == 4 else 16
    so, do = int(rec["src_off"]), int(rec["dst_off"])
    return wc.rx_socktab_lookup(tab, af, frame[do:do + alen], int(rec["dport"]),
                                frame[so:so + alen], int(rec["sport"]))


def expect(buf: np.ndarray, offs, lens, tab: np.ndarray, ns: int, eng, slot_bytes: int):
    """Every output of wc_rx_drain on the CPU, from the models alone."""
    n = len(offs)
    d = dmodel.Expect(buf, offs, lens)
    frames = [buf[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() for i in range(n)]
    sock = np.array([lookup(tab, fr, d.records[i]) for i, fr in enumerate(frames)], np.uint8) \
        .reshape(n)
    lst, start = xmodel.group(sock, ns)
    r = rmodel.Expect(buf, offs, lens, d.verdicts, sock, eng, slot_bytes)
    nb = nmodel.Expect(buf, offs, lens, r.action, eng)
    return SimpleNamespace(
        n=n, frames=frames, verdicts=d.verdicts, records=d.records, drops=d.drops, sock=sock,
        list=lst, start=start, actions=r.action, reply_lens=r.reply_len, reply_list=r.list,
        nact=nb.nact, neigh_reply_list=nb.rlist, update_list=nb.ulist, reply=r, neigh=nb)
