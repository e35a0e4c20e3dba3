#!/usr/bin/env python3
"""RX delivery timed beside the plain RX verdict, in one process.

Over the bench's three netmap rings -- MTU (2^20 frames of 1514 B), mixed
(2^21 frames, Zipf 64-1472 B IP) and mixed with every third frame ARP -- each
in `--rings` distinct device buffers taken in rotation (the frames of one
buffer alone are past the 256 MiB Infinity Cache), these calls alternate, each
between two device events:

    wc_rx_verdict_ragged                       the yardstick
    wc_rx_deliver_ragged with d_list           verdicts + records + list
    wc_rx_select alone (WC_RX_MASK_DELIVER)    the three select launches
    wc_rx_deliver_ragged without d_list        the DELIVER kernel alone

Before timing, every buffer's deliver results are checked against the plain
call's: the same verdicts and drop count, the list = the accepted frames in
order, a zero record exactly where the frame is not accepted.

    python tools/rx_deliver.py [--rounds 8] [--warmup 2] [--rings 2]
    python tools/rx_deliver.py --host-scan     # also: what delivery replaces

--host-scan builds tools/rx_host_scan.c with the C oracle's flags
(oracle/Makefile) and runs it: one core scanning 2^21 verdict bytes and
re-parsing every accepted frame's headers.

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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import warpcore_amd as wc  # noqa: E402
from warpcore_amd import _lib, synth  # noqa: E402

RINGS = (("mtu", 1 << 20, None, 0), ("mixed", 1 << 21, "zipf", 0), ("mixed_arp3", 1 << 21, "zipf", 3))


def build_ring(dev, n, zipf, arp, seed, slot=2048):
    ip_lens = synth.zipf_lengths(n, seed=synth.ZIPF_SEED) if zipf \
        else np.full(n, 1500, dtype=np.uint16)
    buf = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    wc.synth_fill(buf, seed, nbytes=n * slot)
    f_off, f_len = synth.make_rx_ring(buf, n, ip_lens, slot=slot)
    if arp:  # every arp-th frame ARP, as bench.py --rx-arp
        sel = torch.from_numpy(f_off[::arp].astype(np.int64)).to(dev)
        buf[sel + 12] = 0x08
        buf[sel + 13] = 0x06
    return buf, f_off, f_len


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def one_ring(name, n, zipf, arp, args, dev):
    bufs = []
    for r in range(args.rings):
        buf, f_off, f_len = build_ring(dev, n, zipf, arp, 11 + 7 * r)
        bufs.append(buf)
    d_off, d_len = torch.from_numpy(f_off).to(dev), torch.from_numpy(f_len).to(dev)
    nbytes = int(f_len.astype(np.uint64).sum())
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    out2 = torch.empty(n, dtype=torch.uint8, device=dev)
    drops = torch.zeros(1, dtype=torch.int64, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    lst = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(1, wc.rx_select_scratch(n) // 4), dtype=torch.int32, device=dev)
    lib = _lib.active()
    st = torch.cuda.current_stream().cuda_stream

    def call(rc, what):
        if rc:
            raise SystemExit(f"{what}: {rc}")

    def verdict(buf):
        call(lib.wc_rx_verdict_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                      out.data_ptr(), drops.data_ptr(), st), "wc_rx_verdict_ragged")

    def deliver(buf):
        call(lib.wc_rx_deliver_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                      out2.data_ptr(), rec.data_ptr(), lst.data_ptr(),
                                      cnt.data_ptr(), drops.data_ptr(), scratch.data_ptr(), st),
             "wc_rx_deliver_ragged")

    def records(buf):  # the DELIVER kernel alone: no list, no select launches
        call(lib.wc_rx_deliver_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                      out2.data_ptr(), rec.data_ptr(), None, None,
                                      drops.data_ptr(), None, st), "wc_rx_deliver_ragged")

    def select():
        call(lib.wc_rx_select(out.data_ptr(), n, wc.RX_MASK_DELIVER, lst.data_ptr(),
                              cnt.data_ptr(), scratch.data_ptr(), st), "wc_rx_select")

    print(f"== ring {name}: {n} frames, mean {nbytes / n:.1f} B, in 2048-B slots, {args.rings} "
          f"buffers of {n * 2048 / 2**30:.1f} GiB", flush=True)
    for r, buf in enumerate(bufs):
        drops.zero_()
        verdict(buf)
        d_plain = int(drops.item())
        drops.zero_()
        deliver(buf)
        acc = (out == wc.RX_OK) | (out == wc.RX_OK_NO_CKSUM)
        same = bool(torch.equal(out, out2)) and int(drops.item()) == d_plain
        c = int(cnt.item())
        lst_ok = c == int(acc.sum()) and bool(torch.equal(
            lst[:c].to(torch.int64), torch.nonzero(acc).flatten()))
        rec_ok = bool(torch.equal(rec[:, 8] != 0, acc))  # af: 0 exactly where not accepted
        print(f"check, buffer {r}: verdicts and drops equal the plain call's: {same}; list of {c} "
              f"= the accepted frames in order: {lst_ok}; zero records exactly elsewhere: {rec_ok}",
              flush=True)
        if not (same and lst_ok and rec_ok):
            raise SystemExit("deliver check failed")

    tv, td, ts, tr = [], [], [], []
    for i in range(args.warmup + args.rounds):
        buf = bufs[i % args.rings]
        a = timed(lambda: verdict(buf))
        b = timed(lambda: deliver(buf))
        c = timed(select)
        d = timed(lambda: records(buf))
        tag = "warm" if i < args.warmup else "round"
        print(f"{tag} {i:2d}: verdict {a * 1e6:7.1f} us | deliver+list {b * 1e6:7.1f} us "
              f"({b / a:.3f} x) | select alone {c * 1e6:6.1f} us | deliver, no list "
              f"{d * 1e6:7.1f} us", flush=True)
        if i >= args.warmup:
            tv.append(a), td.append(b), ts.append(c), tr.append(d)
    mv, md, ms, mr = (statistics.median(t) for t in (tv, td, ts, tr))
    print(f"== {name}: wc_rx_verdict_ragged median {mv * 1e6:.1f} us (min {min(tv) * 1e6:.1f}); "
          f"wc_rx_deliver_ragged with list median {md * 1e6:.1f} us (min {min(td) * 1e6:.1f}); "
          f"ratio of medians {md / mv:.3f}; wc_rx_select alone median {ms * 1e6:.1f} us "
          f"(min {min(ts) * 1e6:.1f}); wc_rx_deliver_ragged without list median {mr * 1e6:.1f} us "
          f"(min {min(tr) * 1e6:.1f}) over {len(tv)} rounds", flush=True)
    del bufs
    torch.cuda.empty_cache()


def host_scan():
    flags = ["-Ofast", "-march=native", "-std=gnu11", "-Wall", "-Wextra"]  # oracle/Makefile CFLAGS
    with tempfile.TemporaryDirectory(prefix="wc-hostscan-") as tmp:
        exe = Path(tmp) / "rx_host_scan"
        subprocess.run(["gcc", *flags, str(ROOT / "tools" / "rx_host_scan.c"), "-o", str(exe)],
                       check=True)
        for arp in ("0", "3"):
            r = subprocess.run([str(exe), str(1 << 21), arp], check=True, capture_output=True,
                               text=True)
            print(r.stdout.strip(), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=2)
    ap.add_argument("--only", default="", help="one ring: mtu, mixed or mixed_arp3")
    ap.add_argument("--host-scan", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    for name, n, zipf, arp in RINGS:
        if not args.only or args.only == name:
            one_ring(name, n, zipf, arp, args, dev)
    print("(device-event times of single calls; kernel times: rocprofv3 --kernel-trace --stats)")
    if args.host_scan:
        host_scan()


if __name__ == "__main__":
    main()
