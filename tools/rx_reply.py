#!/usr/bin/env python3
"""RX replies timed beside the RX chain in front of them, in one process.

A ring of `--frames` Ethernet frames in 2048-byte slots (`--rings` distinct
device buffers taken in rotation) is tiled from 1024 host-built templates:
one frame in `--every` is an ICMP / ICMPv6 echo request (payload sizes drawn
from 0..1472, every fourth IPv6), one a TCP segment (a scan: protocol
unreachable), one a UDP datagram for an unbound port from one of our own
addresses (port unreachable); the rest are UDP datagrams for the one bound
socket.  `--every 1` is the flood: no bound UDP at all.  These calls
alternate, each between two device events:

    wc_rx_deliver_ragged (no list) + wc_rx_demux (ids)   the chain in front
    wc_rx_reply_plan with its list                        four launches
    wc_rx_reply_plan without the list                     the plan kernel
    wc_rx_reply_build                                     one launch

Before timing, the device's actions, reply count and built count are checked
against the classes the ring was built from.

    python tools/rx_reply.py [--frames 262144] [--every 8] [--rounds 8] [--warmup 2] [--rings 2]

For kernel times run the same command under `rocprofv3 --kernel-trace --stats`,
as a run of its own.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import warpcore_amd as wc  # noqa: E402
from rx_deliver import timed  # noqa: E402

SLOT, TEMPLATES = 2048, 1024
MAC, PEER_MAC = bytes((2, 0, 0, 0, 0, 1)), bytes((2, 0, 0, 0, 0, 9))
A4, A6 = bytes((10, 1, 0, 1)), bytes.fromhex("fe80000000000000020000fffe000001")
PEER4, PEER6 = bytes((192, 168, 7, 7)), bytes.fromhex("20010db8000000000000000000000099")
PORT = 4433


def csum(b: bytes, init: int = 0) -> bytes:
    """in_cksum.c:107-137 on the host, stored raw."""
    a = np.frombuffer(b + b"\x00" * (len(b) & 1), "<u2").astype(np.uint64)
    s = int(a.sum()) + init
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    s = ~s & 0xFFFF
    return bytes((s & 0xFF, s >> 8))


def ip4(payload: bytes, proto: int, src: bytes = PEER4) -> bytes:
    h = b"\x45\x00" + (20 + len(payload)).to_bytes(2, "big") + b"\x12\x34\x40\x00" + \
        bytes((64, proto)) + b"\x00\x00" + src + A4
    return h[:10] + csum(h) + h[12:] + payload


def template(kind: str, rng) -> bytes:
    data = rng.integers(0, 256, int(rng.integers(0, 1473)), dtype=np.uint8).tobytes()
    if kind == "echo4":
        m = b"\x08\x00\x00\x00\xab\xcd\x00\x01" + data
        return MAC + PEER_MAC + b"\x08\x00" + ip4(m[:2] + csum(m) + m[4:], 1)
    if kind == "echo6":
        m = b"\x80\x00\x00\x00\xab\xcd\x00\x01" + data[:1452]
        h = b"\x60\x00\x00\x00" + len(m).to_bytes(2, "big") + b"\x3a\x40" + PEER6 + A6
        ck = csum(h[8:40] + h[4:6] + m, 58 << 24)
        return MAC + PEER_MAC + b"\x86\xdd" + h + m[:2] + ck + m[4:]
    if kind == "tcp":
        return MAC + PEER_MAC + b"\x08\x00" + ip4(data[:40] + bytes(20), 6)
    port = PORT if kind == "udp" else 9  # "unbound": from our own address (udp.c:150)
    u = b"\x9c\x40" + port.to_bytes(2, "big") + (8 + len(data)).to_bytes(2, "big") + b"\x00\x00" + data
    return MAC + PEER_MAC + b"\x08\x00" + ip4(u, 17, A4 if kind == "unbound" else PEER4)


def build_ring(dev, n: int, every: int, seed: int):
    rng = np.random.default_rng(seed)
    kinds = []
    for t in range(TEMPLATES):
        k = t % (3 * every)
        kinds.append(("echo6" if (t // (3 * every)) % 4 == 3 else "echo4") if k == 0 else
                     "tcp" if k == every else "unbound" if k == 2 * every else "udp")
    if every == 1:
        kinds = [("echo6" if t % 4 == 3 else "echo4") for t in range(TEMPLATES)]
    block = np.zeros((TEMPLATES, SLOT), np.uint8)
    lens = np.empty(TEMPLATES, np.uint16)
    for t, kind in enumerate(kinds):
        fr = template(kind, rng)
        block[t, :len(fr)], lens[t] = np.frombuffer(fr, np.uint8), len(fr)
    reps = n // TEMPLATES
    buf = torch.from_numpy(block.reshape(-1)).to(dev).repeat(reps)
    buf = torch.cat([buf, torch.zeros(64, dtype=torch.uint8, device=dev)])
    f_off = (np.arange(n, dtype=np.uint64) * SLOT)
    return buf, f_off, np.tile(lens, reps), np.array(kinds * reps)


def engine() -> np.ndarray:
    e = np.zeros(1, wc.RX_ENGINE)
    e["mac"][0], e["mtu"], e["naddr"] = np.frombuffer(MAC, np.uint8), 1500, 2
    e["addr"][0][0]["af"], e["addr"][0][1]["af"] = 6, 4
    e["addr"][0][0]["addr"][:] = np.frombuffer(A6, np.uint8)
    e["addr"][0][1]["addr"][:4] = np.frombuffer(A4, np.uint8)
    wc.rx_engine_check(e)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    n = args.frames // TEMPLATES * TEMPLATES
    rings = [build_ring(dev, n, args.every, 11 + 7 * r) for r in range(args.rings)]
    socks = np.zeros(1, wc.RX_SOCK)
    socks["af"], socks["lport"] = 4, ((PORT & 0xFF) << 8) | (PORT >> 8)
    socks["laddr"][0][:4] = np.frombuffer(A4, np.uint8)
    tab = torch.from_numpy(wc.rx_socktab_build(socks)).to(dev)
    eng = torch.from_numpy(engine().view(np.uint8)).to(dev)
    _, f_off, _, kinds = rings[0]
    d_off = torch.from_numpy(f_off).to(dev)
    d_lens = [torch.from_numpy(r[2]).to(dev) for r in rings]
    want = int(np.isin(kinds, ("echo4", "echo6", "tcp", "unbound")).sum())
    out = torch.empty(want * SLOT + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(want, dtype=torch.int64, device=dev) * SLOT
    state = {}

    def front(r):
        v, rec, _, _, _ = wc.rx_deliver_ragged(rings[r][0], d_off, d_lens[r], want_list=False,
                                               check=False)
        sock, _, _ = wc.rx_demux(rings[r][0], d_off, rec, tab, 1, want_list=False)
        state[r] = (v, sock)

    def plan(r, want_list=True):
        v, sock = state[r]
        state[r, "plan"] = wc.rx_reply_plan(rings[r][0], d_off, d_lens[r], v, sock, eng, SLOT,
                                            want_list=want_list, check=False)

    def build(r):
        act, _, lst, cnt = state[r, "plan"]
        state[r, "built"] = wc.rx_reply_build(rings[r][0], d_off, d_lens[r], act, lst, cnt, eng, out,
                                              o_off, SLOT, check=False)

    print(f"== {n} frames in {SLOT}-B slots, {args.rings} buffers; one echo, one TCP and one "
          f"unbound UDP frame in {3 * args.every}" if args.every > 1 else
          f"== {n} frames in {SLOT}-B slots, {args.rings} buffers; every frame an echo request",
          flush=True)
    for r in range(args.rings):
        front(r), plan(r), build(r)
        act, rlen, _, cnt = state[r, "plan"]
        a = act.cpu().numpy()
        k = rings[r][3]
        exp = np.select([k == "echo4", k == "echo6", k == "tcp", k == "unbound"],
                        [wc.RR_ECHO4, wc.RR_ECHO6, wc.RR_UNREACH_PROTO4, wc.RR_UNREACH_PORT4],
                        wc.RR_NONE)
        ok = bool((a == exp).all()) and int(cnt.item()) == want and \
            int(state[r, "built"][1].item()) == want
        icmp = int(rings[r][2][np.isin(k, ("echo4", "echo6"))].astype(np.int64).sum())
        wrote = int(rlen.cpu().numpy().astype(np.int64).sum())
        print(f"check, buffer {r}: {want} replies planned and built, actions equal the classes: "
              f"{ok}; {icmp} echo-frame bytes, {wrote} reply bytes", flush=True)
        if not ok:
            raise SystemExit("reply check failed")
    ts = {k: [] for k in ("front", "plan", "plan_only", "build")}
    for i in range(args.warmup + args.rounds):
        r = i % args.rings
        t = {"front": timed(lambda: front(r)), "plan": timed(lambda: plan(r)),
             "build": timed(lambda: build(r)), "plan_only": timed(lambda: plan(r, False))}
        plan(r)
        tag = "warm" if i < args.warmup else "round"
        print(f"{tag} {i:2d}: deliver + demux {t['front'] * 1e6:7.1f} us | plan + list "
              f"{t['plan'] * 1e6:7.1f} us | plan alone {t['plan_only'] * 1e6:7.1f} us | build "
              f"{t['build'] * 1e6:7.1f} us", flush=True)
        if i >= args.warmup:
            for k in ts:
                ts[k].append(t[k])
    med = {k: statistics.median(v) for k, v in ts.items()}
    print(f"== medians over {args.rounds} rounds: deliver + demux {med['front'] * 1e6:.1f} us (min "
          f"{min(ts['front']) * 1e6:.1f}); plan + list {med['plan'] * 1e6:.1f} us (min "
          f"{min(ts['plan']) * 1e6:.1f}); plan alone {med['plan_only'] * 1e6:.1f} us (min "
          f"{min(ts['plan_only']) * 1e6:.1f}); build {med['build'] * 1e6:.1f} us (min "
          f"{min(ts['build']) * 1e6:.1f}): {wrote / med['build'] / 1e9:.1f} GB/s of reply bytes written; "
          f"plan + build = {(med['plan'] + med['build']) / med['front']:.2f} x the chain in front",
          flush=True)
    print("(device-event times of single calls, Python wrappers and their allocations included; "
          "kernel times: rocprofv3 --kernel-trace --stats)")


if __name__ == "__main__":
    main()
