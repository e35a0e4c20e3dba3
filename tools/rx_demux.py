#!/usr/bin/env python3
"""RX socket demultiplex timed beside RX delivery, in one process.

Over the bench's three netmap rings -- MTU (2^20 frames of 1514 B), mixed
(2^21 frames, Zipf 64-1472 B IP) and mixed with every third frame ARP -- each
in `--rings` distinct device buffers taken in rotation, and for tables of 1, 16
and 254 sockets, these calls alternate, each between two device events:

    wc_rx_deliver_ragged with d_list                 the comparator (delivery as it was)
    wc_rx_deliver_ragged without d_list, wc_rx_demux the demultiplexed delivery
    wc_rx_demux alone, with lists                    the three demux launches
    wc_rx_demux alone, ids only                      the key kernel

The frames are made to hit the table: frame i's destination address and port
are those of a socket of its IP version, chosen uniformly by a hash of i (every
second socket is connected, and then the source is its remote too), and the
ring is sealed again with wc_tx_seal_ragged, so every frame still verifies.
With one socket (IPv4) the IPv6 frames stay unbound.  `--unbound 8` leaves
every 8th frame as it was: no socket takes it.

Before timing, every buffer's result is checked on the host: each delivered
frame's id is the socket it was aimed at, the list is the stable grouping of
those ids and the starts are its run boundaries.

    python tools/rx_demux.py [--rounds 8] [--warmup 2] [--rings 2] [--socks 1,16,254]
    python tools/rx_demux.py --host-demux    # also: what the call replaces
    python tools/rx_demux.py --only none --host-demux    # that alone

--host-demux builds tools/rx_host_demux.c with the C oracle's flags and runs
it: one core walking the delivered list, reading both addresses through the
record, wc_rx_socktab_lookup, append.

For kernel times run the same command under `rocprofv3 --kernel-trace --stats`,
as a run of its own.
"""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import warpcore_amd as wc  # noqa: E402
from rx_deliver import RINGS, build_ring, timed  # noqa: E402
from warpcore_amd import _lib  # noqa: E402


def make_socks(ns: int) -> np.ndarray:
    """ns sockets: every third IPv6, every second connected, distinct tuples."""
    s = np.zeros(ns, dtype=wc.RX_SOCK)
    rng = np.random.default_rng(ns)
    for j in range(ns):
        s["af"][j] = 6 if j % 3 == 2 else 4
        s["connected"][j] = j & 1
        s["laddr"][j] = rng.integers(0, 256, 16)
        s["raddr"][j] = rng.integers(0, 256, 16)
        s["lport"][j], s["rport"][j] = 1024 + j, 40000 + j
    return s


def aim(buf, f_off, socks, unbound_every: int):
    """Point the ring's frames at the sockets (see the module text); returns
    the socket each frame was aimed at (RX_SOCK_UNBOUND: left as it was)."""
    n, dev = f_off.size, buf.device
    i = np.arange(n, dtype=np.uint64)
    v6 = i % 3 == 0  # synth.make_rx_ring's versions
    pick = ((i * np.uint64(2654435761)) >> np.uint64(8)).astype(np.int64)
    want = np.full(n, wc.RX_SOCK_UNBOUND, dtype=np.uint8)
    for af, sel in ((4, ~v6), (6, v6)):
        ids = np.flatnonzero(socks["af"] == af)
        if ids.size == 0:
            continue
        take = sel & ((i % np.uint64(unbound_every) != 5) if unbound_every else True)
        at = np.flatnonzero(take)
        j = ids[pick[at] % ids.size]
        want[at] = j
        alen = 4 if af == 4 else 16
        src, dst, udp = (12, 16, 20) if af == 4 else (8, 24, 40)
        base = torch.from_numpy(f_off[at].astype(np.int64) + 14).to(dev)

        def put(where, rows, who=None):
            b, r = (base, rows) if who is None else (base[who], rows[who.cpu().numpy()])
            cols = torch.arange(r.shape[1], device=dev)
            buf[(b[:, None] + where + cols[None, :]).reshape(-1)] = \
                torch.from_numpy(np.ascontiguousarray(r)).to(dev).reshape(-1)
        put(dst, socks["laddr"][j][:, :alen])
        put(udp + 2, socks["lport"][j].astype("<u2").view(np.uint8).reshape(-1, 2))
        conn = torch.from_numpy(socks["connected"][j] == 1).to(dev)
        put(src, socks["raddr"][j][:, :alen], conn)
        put(udp, socks["rport"][j].astype("<u2").view(np.uint8).reshape(-1, 2), conn)
    return want


def one_ring(name, n, zipf, arp, ns, args, dev):
    socks = make_socks(ns)
    tab = torch.from_numpy(wc.rx_socktab_build(socks)).to(dev)
    bufs, wants = [], []
    for r in range(args.rings):
        buf, f_off, f_len = build_ring(dev, n, zipf, arp, 11 + 7 * r)
        wants.append(aim(buf, f_off, socks, args.unbound))
        bufs.append(buf)
    d_off, d_len = torch.from_numpy(f_off).to(dev), torch.from_numpy(f_len).to(dev)
    for buf in bufs:
        wc.tx_seal_ragged(buf, d_off, d_len, check=False)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    drops = torch.zeros(1, dtype=torch.int64, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    lst = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    sock = torch.empty(n, dtype=torch.uint8, device=dev)
    start = torch.zeros(256, dtype=torch.int64, device=dev)
    sel_scratch = torch.empty(max(1, wc.rx_select_scratch(n) // 4), dtype=torch.int32, device=dev)
    dmx_scratch = torch.empty(max(1, wc.rx_demux_scratch(n) // 4), dtype=torch.int32, device=dev)
    lib = _lib.active()
    st = torch.cuda.current_stream().cuda_stream

    def call(rc, what):
        if rc:
            raise SystemExit(f"{what}: {rc}")

    def deliver(buf, with_list):
        call(lib.wc_rx_deliver_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                      out.data_ptr(), rec.data_ptr(),
                                      lst.data_ptr() if with_list else None,
                                      cnt.data_ptr() if with_list else None, drops.data_ptr(),
                                      sel_scratch.data_ptr() if with_list else None, st),
             "wc_rx_deliver_ragged")

    def demux(buf, with_list=True):
        call(lib.wc_rx_demux(buf.data_ptr(), d_off.data_ptr(), rec.data_ptr(), n, tab.data_ptr(),
                             ns, sock.data_ptr(), lst.data_ptr() if with_list else None,
                             start.data_ptr() if with_list else None,
                             dmx_scratch.data_ptr() if with_list else None, st), "wc_rx_demux")

    print(f"== ring {name}, {ns} sockets" + (f", every {args.unbound}th frame unbound"
                                             if args.unbound else "") +
          f": {n} frames in 2048-B slots, {args.rings} buffers", flush=True)
    for r, buf in enumerate(bufs):
        deliver(buf, False)
        demux(buf)
        v = out.cpu().numpy()
        acc = (v == wc.RX_OK) | (v == wc.RX_OK_NO_CKSUM)
        want = np.where(acc, wants[r], wc.RX_SOCK_NONE).astype(np.uint8)
        got = sock.cpu().numpy()
        ids_ok = bool((got == want).all())
        key = np.where(want == wc.RX_SOCK_UNBOUND, ns, want.astype(np.int64))
        d = np.flatnonzero(acc)
        order = d[np.argsort(key[d], kind="stable")]
        hist = np.bincount(key[d], minlength=ns + 1)[:ns + 1]
        w_start = np.zeros(256, np.int64)
        w_start[:ns + 1] = np.concatenate([[0], np.cumsum(hist)[:-1]])
        w_start[ns:255] = w_start[ns]
        w_start[255] = d.size
        g_start = start.cpu().numpy()
        lst_ok = bool((lst[:d.size].cpu().numpy().view(np.uint32) == order).all())
        print(f"check, buffer {r}: {d.size} delivered, {int((want == wc.RX_SOCK_UNBOUND).sum())} "
              f"unbound; ids equal the sockets aimed at: {ids_ok}; list = the stable grouping: "
              f"{lst_ok}; starts: {bool((g_start == w_start).all())}", flush=True)
        if not (ids_ok and lst_ok and (g_start == w_start).all()):
            raise SystemExit("demux check failed")

    ta, tb, tc, td = [], [], [], []
    for i in range(args.warmup + args.rounds):
        buf = bufs[i % args.rings]
        a = timed(lambda: deliver(buf, True))
        b = timed(lambda: (deliver(buf, False), demux(buf)))
        c = timed(lambda: demux(buf))
        d = timed(lambda: demux(buf, False))
        tag = "warm" if i < args.warmup else "round"
        print(f"{tag} {i:2d}: deliver+list {a * 1e6:7.1f} us | deliver, no list + demux "
              f"{b * 1e6:7.1f} us ({b / a:.3f} x) | demux alone {c * 1e6:6.1f} us | ids only "
              f"{d * 1e6:6.1f} us", flush=True)
        if i >= args.warmup:
            ta.append(a), tb.append(b), tc.append(c), td.append(d)
    ma, mb, mc, md = (statistics.median(t) for t in (ta, tb, tc, td))
    print(f"== {name}, {ns} sockets: wc_rx_deliver_ragged with list median {ma * 1e6:.1f} us (min "
          f"{min(ta) * 1e6:.1f}); without list + wc_rx_demux median {mb * 1e6:.1f} us (min "
          f"{min(tb) * 1e6:.1f}); ratio of medians {mb / ma:.3f}; wc_rx_demux alone median "
          f"{mc * 1e6:.1f} us (min {min(tc) * 1e6:.1f}); ids only median {md * 1e6:.1f} us (min "
          f"{min(td) * 1e6:.1f}) over {len(ta)} rounds", flush=True)
    del bufs
    torch.cuda.empty_cache()


def host_demux(socks_list):
    flags = ["-Ofast", "-march=native", "-std=gnu11", "-Wall", "-Wextra"]  # oracle/Makefile CFLAGS
    with tempfile.TemporaryDirectory(prefix="wc-hostdemux-") as tmp:
        exe = Path(tmp) / "rx_host_demux"
        subprocess.run(["gcc", *flags, f"-I{ROOT / 'include'}", str(ROOT / "tools" / "rx_host_demux.c"),
                        "-o", str(exe), f"-L{ROOT / 'warpcore_amd'}", "-lwccksum",
                        "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{ROOT / 'warpcore_amd'}"],
                       check=True)
        for ns in socks_list:
            r = subprocess.run([str(exe), str(1 << 21), str(ns)], check=True, capture_output=True,
                               text=True)
            print(r.stdout.strip(), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=2)
    ap.add_argument("--only", default="", help="one ring: mtu, mixed or mixed_arp3")
    ap.add_argument("--socks", default="1,16,254")
    ap.add_argument("--unbound", type=int, default=0, help="leave every N-th frame unbound")
    ap.add_argument("--host-demux", action="store_true")
    args = ap.parse_args()
    socks_list = [int(x) for x in args.socks.split(",") if x]
    if not args.host_demux or args.only != "none":
        dev = torch.device("cuda:0")
        wc.gpu_init(0)
        for name, n, zipf, arp in RINGS:
            if not args.only or args.only == name:
                for ns in socks_list:
                    one_ring(name, n, zipf, arp, ns, args, dev)
        print("(device-event times of single calls; kernel times: rocprofv3 --kernel-trace --stats)")
    if args.host_demux:
        host_demux(socks_list)


if __name__ == "__main__":
    main()
