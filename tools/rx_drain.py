#!/usr/bin/env python3
"""wc_rx_drain timed against the four-call chain it stands for, in one process
and from the same build (the chain is unchanged code).

For n = 64, 256, 1024 and 4096 frames, on two rings in 2048-byte slots:

    mixed   the world of tests/rx_drain_cases.py (ARP and neighbour discovery,
            ICMP of both families, UDP for bound, connected and unbound ports),
            600 host-built frames tiled to n
    mtu     1472-byte UDP datagrams to bound sockets

both paths are called through the C ABI on preallocated outputs (no Python
wrapper, no allocation inside the timed region):

    drain   wc_rx_drain                                        2 launches
    chain   wc_rx_deliver_ragged, wc_rx_demux, wc_rx_reply_plan,
            wc_rx_neigh_plan with every list                   17 launches

Each timing is the host's clock around one call (the chain: its four) and one
synchronize; the figure is the median of `--calls` (at least 200) after
`--warmup`, with the minimum and maximum.  Before timing, every output of the
drain is compared with the chain's.

    python tools/rx_drain.py [--calls 300] [--warmup 50] [--sizes 64,256,1024,4096]
"""
from __future__ import annotations

import argparse
import ctypes
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rx_drain_cases as cases  # noqa: E402
import rx_reply_cases as rc  # noqa: E402
import warpcore_amd as wc  # noqa: E402
from packets import finish_udp, ipv4_udp  # noqa: E402
from warpcore_amd import _lib  # noqa: E402
from warpcore_amd.cksum import _DrainOut  # noqa: E402

SLOT = 2048
PER_FRAME = {"verdict": 1, "rec": 16, "sock": 1, "action": 1, "reply_len": 2, "nact": 1}
LISTS = {"list": "start", "rlist": "rcount", "nrlist": "nrcount", "ulist": "ucount"}


def mtu_frame(rng, s) -> bytes:
    """A 1472-byte datagram for the bound IPv4 socket `s`, to our MAC."""
    payload = rng.integers(0, 256, 1472, dtype=np.uint8).tobytes()
    b = bytearray(ipv4_udp(payload, rng)[0])
    b[12:16], b[16:20] = rc.PEER4, bytes(s["laddr"][:4])
    b[20:24] = int(rng.integers(1, 1 << 16)).to_bytes(2, "little") + int(s["lport"]).to_bytes(2, "little")
    return rc.MAC + rc.PEER_MAC + b"\x08\x00" + finish_udp(bytes(b))


def ring(dev, frames, n: int):
    """n slots over the base frames in turn: (buffer, offsets, lengths)."""
    m = len(frames)
    block = np.zeros((m, SLOT), np.uint8)
    for t, fr in enumerate(frames):
        block[t, :len(fr)] = np.frombuffer(fr, np.uint8)
    idx = np.arange(n) % m
    buf = torch.from_numpy(block[idx].reshape(-1)).to(dev)
    buf = torch.cat([buf, torch.zeros(64, dtype=torch.uint8, device=dev)])
    lens = np.array([len(frames[i]) for i in idx], np.uint16)
    return buf, torch.from_numpy(np.arange(n, dtype=np.uint64) * SLOT).to(dev), torch.from_numpy(lens).to(dev)


class Outputs:
    """One set of the fifteen arrays, and the struct that names them."""

    def __init__(self, dev, n: int):
        t = {k: torch.zeros(n * w, dtype=torch.uint8, device=dev) for k, w in PER_FRAME.items()}
        t.update({k: torch.zeros(n, dtype=torch.int32, device=dev) for k in LISTS})
        t.update({k: torch.zeros(1, dtype=torch.int64, device=dev)
                  for k in ("drops", "rcount", "nrcount", "ucount")})
        t["start"] = torch.zeros(256, dtype=torch.int64, device=dev)
        self.t = t
        self.p = {k: v.data_ptr() for k, v in t.items()}
        self.c = _DrainOut(**self.p)

    def host(self):
        h = {k: self.t[k].cpu().numpy() for k in PER_FRAME}
        h["starts"] = self.t["start"].cpu().numpy()
        for k, c in LISTS.items():
            cnt = int(self.t[c][255 if c == "start" else 0].item())
            h[k], h[c] = self.t[k].cpu().numpy()[:cnt], cnt  # (h["start"]: the delivered count)
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--sizes", default="64,256,1024,4096")
    args = ap.parse_args()
    if args.calls < 200:
        raise SystemExit("--calls: at least 200")
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    lib = _lib.active()
    seed, _, ns, slot = cases.WORLDS["slots"]
    frames, socks = cases.world(seed, 600, ns)
    rng = np.random.default_rng(seed)
    bound4 = [s for s in socks if int(s["af"]) == 4 and not int(s["connected"])]
    rings = {"mixed": frames, "mtu": [mtu_frame(rng, bound4[k % len(bound4)]) for k in range(64)]}
    d_tab = torch.from_numpy(wc.rx_socktab_build(socks).view(np.uint8).copy()).to(dev)
    d_eng = torch.from_numpy(rc.engine_table().view(np.uint8).reshape(-1).copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    print(f"== wc_rx_drain against the four-call chain: {args.calls} calls after {args.warmup}, one "
          f"synchronize per call; {ns} sockets, slot_bytes {slot}; WC_RX_DRAIN_SMALL = "
          f"{wc.RX_DRAIN_SMALL}", flush=True)
    for name, base in rings.items():
        for n in [int(x) for x in args.sizes.split(",")]:
            buf, d_off, d_len = ring(dev, base, n)
            a, b = Outputs(dev, n), Outputs(dev, n)
            scratch = torch.zeros(wc.rx_drain_scratch(n) // 4 + 1, dtype=torch.int32, device=dev)
            bp, op, lp, tp, ep, sp = (buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                      d_tab.data_ptr(), d_eng.data_ptr(), scratch.data_ptr())

            def drain():
                return lib.wc_rx_drain(bp, op, lp, n, tp, ns, ep, slot, ctypes.byref(a.c), sp, st)

            def chain():
                p = b.p
                return (lib.wc_rx_deliver_ragged(bp, op, lp, n, p["verdict"], p["rec"], None, None,
                                                 p["drops"], None, st)
                        or lib.wc_rx_demux(bp, op, p["rec"], n, tp, ns, p["sock"], p["list"], p["start"],
                                           sp, st)
                        or lib.wc_rx_reply_plan(bp, op, lp, n, p["verdict"], p["sock"], ep, slot,
                                                p["action"], p["reply_len"], p["rlist"], p["rcount"],
                                                sp, st)
                        or lib.wc_rx_neigh_plan(bp, op, lp, n, p["action"], ep, p["nact"], p["nrlist"],
                                                p["nrcount"], p["ulist"], p["ucount"], sp, st))

            if drain() or chain():
                raise SystemExit("a call failed")
            torch.cuda.synchronize()
            ha, hb = a.host(), b.host()
            same = all(np.array_equal(ha[k], hb[k]) for k in ha)
            print(f"check, {name} n = {n}: the drain's fifteen outputs equal the chain's: {same} "
                  f"({hb['start']} delivered, {hb['rcount']} replies, {hb['nrcount']} neighbour replies, "
                  f"{hb['ucount']} updates)", flush=True)
            if not same:
                raise SystemExit("drain check failed")
            ts = {"drain": [], "chain": []}
            for i in range(args.warmup + args.calls):
                for k, f in (("drain", drain), ("chain", chain)):
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        ts[k].append(time.perf_counter() - t0)
            md, mc = statistics.median(ts["drain"]), statistics.median(ts["chain"])
            print(f"{name:5s} n = {n:4d}: drain {md * 1e6:7.1f} us ({min(ts['drain']) * 1e6:.1f} .. "
                  f"{max(ts['drain']) * 1e6:.1f}) | chain {mc * 1e6:7.1f} us "
                  f"({min(ts['chain']) * 1e6:.1f} .. {max(ts['chain']) * 1e6:.1f}) | chain / drain "
                  f"{mc / md:.2f}", flush=True)
    print("(host clock around one call and one synchronize, both paths through the C ABI on "
          "preallocated outputs)")


if __name__ == "__main__":
    main()
