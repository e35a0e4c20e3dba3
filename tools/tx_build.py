#!/usr/bin/env python3
"""The TX build timed beside the TX seal on the same MTU ring.

The ring is tools/tx_seal.py's shape: 2^20 frames in 2048-B slots,
device-resident, `--rings` distinct buffers (each 2 GiB, far past the 256 MiB
Infinity Cache) taken in rotation, 2:1 IPv4 / IPv6, every payload 1472 random
bytes (frames of 1514 and 1534 B), 16 connected sockets.  Every buffer is
first built once and checked: all frames SEALED, every RX verdict OK or
OK_NO_CKSUM.  In one process wc_tx_build_ragged and wc_tx_seal_ragged then
alternate over the rings, each call between two device events; per call the
frame bytes over the event time.  The seal is the comparator: the build reads
no header and has no dependent parse round, so its median is expected to be at
most the seal's median plus the seal's own spread (max - min) over the pairs
of the run.

    python tools/tx_build.py [--pairs 8] [--warmup 2] [--rings 2] [--packets N]
    python tools/tx_build.py --host [--reps 3]

--host: the host calls over the same frames in host memory, registered and
pageable: wc_tx_build_host against wc_tx_seal_host on headers already written,
wall-clock per call.

For kernel times run the same command under `rocprofv3 --kernel-trace --stats`.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import warpcore_amd as wc  # noqa: E402
from warpcore_amd import _lib  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes / s
SLOT, DATA_LEN, NSOCKS = 2048, 1472, 16


def tables(n, seed=5):
    """16 connected sockets (even index IPv4, odd IPv6; every other pair with
    the ECN default) and one descriptor per frame: every third frame IPv6."""
    rng = np.random.default_rng(seed)
    socks = np.frombuffer(rng.integers(0, 256, NSOCKS * wc.TX_SOCK.itemsize,
                                       dtype=np.uint8).tobytes(), dtype=wc.TX_SOCK).copy()
    k = np.arange(NSOCKS)
    socks["af"] = np.where(k & 1, 6, 4)
    socks["flags"] = wc.TX_SOCK_CONNECTED | np.where(k & 2, wc.TX_SOCK_ECN, 0)
    wc.tx_socks_check(socks)
    i = np.arange(n)
    descs = np.zeros(n, dtype=wc.TX_DESC)
    descs["data_len"] = DATA_LEN
    descs["ip_id"] = rng.integers(0, 65536, n)
    descs["sock"] = 2 * ((i // 3) % (NSOCKS // 2)) + (i % 3 == 0)
    descs["tos"] = np.array((0, 0xB8, 1, 0xBB), np.uint8)[(i // 5) % 4]
    f_off = (i.astype(np.uint64) * np.uint64(SLOT)).astype(np.uint64)
    f_len = np.where(i % 3 == 0, 62 + DATA_LEN, 42 + DATA_LEN).astype(np.uint16)
    return socks, descs, f_off, f_len


def device_pairs(args):
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    n = args.packets
    socks, descs, f_off, f_len = tables(n)
    rings = []
    for r in range(args.rings):
        buf = torch.empty(n * SLOT + 64, dtype=torch.uint8, device=dev)
        wc.synth_fill(buf, 11 + 7 * r, nbytes=n * SLOT)
        rings.append(buf)
    d_off = torch.from_numpy(f_off).to(dev)
    d_len = torch.from_numpy(f_len).to(dev)
    d_desc = torch.from_numpy(descs.view(np.uint8)).to(dev)
    d_socks = torch.from_numpy(socks.view(np.uint8)).to(dev)
    nbytes = int(f_len.astype(np.uint64).sum())
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    flen_out = torch.empty(n, dtype=torch.uint16, device=dev)
    errors = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = _lib.active()
    stream = torch.cuda.current_stream().cuda_stream

    def build(buf):  # the C calls themselves: nothing allocated between the events
        rc = lib.wc_tx_build_ragged(buf.data_ptr(), d_off.data_ptr(), d_desc.data_ptr(), n,
                                    d_socks.data_ptr(), NSOCKS, None, 0, SLOT, 0,
                                    flen_out.data_ptr(), status.data_ptr(), None, None,
                                    errors.data_ptr(), stream)
        if rc:
            raise SystemExit(f"wc_tx_build_ragged: {rc}")

    def seal(buf):
        rc = lib.wc_tx_seal_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, 0,
                                   status.data_ptr(), None, None, errors.data_ptr(), stream)
        if rc:
            raise SystemExit(f"wc_tx_seal_ragged: {rc}")

    print(f"ring: {n} frames of {nbytes / n:.0f} B (data_len {DATA_LEN}) in {SLOT}-B slots, "
          f"{args.rings} buffers of {n * SLOT / 2**30:.1f} GiB, {NSOCKS} connected sockets",
          flush=True)

    # the built-ring check, on every buffer's first build
    for r, buf in enumerate(rings):
        fl, st, _, _, errs = wc.tx_build_ragged(buf, d_off, d_desc, d_socks, None, SLOT)
        v, _ = wc.rx_verdict_ragged(buf, d_off, d_len, check=r == 0)
        sealed = int((st == wc.TX_SEALED).sum())
        same_len = bool(torch.equal(fl.view(torch.int16), d_len.view(torch.int16)))
        ok = int(((v == wc.RX_OK) | (v == wc.RX_OK_NO_CKSUM)).sum())
        print(f"built-ring check, buffer {r}: {sealed} of {n} SEALED, {int(errs.item())} errors, "
              f"frame lengths as expected: {same_len}; RX verdicts OK or OK_NO_CKSUM: {ok} of {n}",
              flush=True)
        if sealed != n or ok != n or not same_len:
            raise SystemExit("built-ring check failed")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    build_t, seal_t = [], []
    for i in range(args.warmup + args.pairs):
        buf = rings[i % args.rings]
        tb = timed(lambda: build(buf))
        ts = timed(lambda: seal(buf))
        tag = "warm" if i < args.warmup else "pair"
        print(f"{tag} {i:2d}: build {tb * 1e6:8.1f} us {nbytes / tb / 1e12:6.3f} TB/s "
              f"({nbytes / tb / PEAK:.3f} of peak) | seal {ts * 1e6:8.1f} us "
              f"{nbytes / ts / 1e12:6.3f} TB/s ({nbytes / ts / PEAK:.3f} of peak)", flush=True)
        if i >= args.warmup:
            build_t.append(tb)
            seal_t.append(ts)
    for name, ts in (("wc_tx_build_ragged", build_t), ("wc_tx_seal_ragged", seal_t)):
        rate = [nbytes / t / PEAK for t in ts]
        print(f"== {name}: median {statistics.median(ts) * 1e6:.1f} us, "
              f"{statistics.median(rate):.3f} of peak over the frame bytes "
              f"(min {min(ts) * 1e6:.1f} us, max {max(ts) * 1e6:.1f} us) over {len(ts)} calls",
              flush=True)
    mb, ms = statistics.median(build_t), statistics.median(seal_t)
    spread = max(seal_t) - min(seal_t)
    met = mb <= ms + spread
    print(f"== expectation: build median {mb * 1e6:.1f} us <= seal median {ms * 1e6:.1f} us + seal "
          f"spread {spread * 1e6:.1f} us = {(ms + spread) * 1e6:.1f} us: "
          f"{'met' if met else 'MISSED'}", flush=True)
    print("(device-event times of single calls; kernel times: rocprofv3 --kernel-trace --stats)")


def host_calls(args):
    wc.gpu_init(0)
    n = args.packets
    socks, descs, f_off, f_len = tables(n)
    rng = np.random.default_rng(23)
    raw = rng.integers(0, 256, n * SLOT + 64, dtype=np.uint8)
    nbytes = int(f_len.astype(np.uint64).sum())
    for registered in (True, False):
        a, b = raw.copy(), raw.copy()
        # b: headers already written (one build), then sealed again and again
        wc.tx_build_host(b, f_off, descs, socks, None, SLOT)
        if registered:
            wc.host_register(a)
            wc.host_register(b)
        ts_build, ts_seal = [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            flen, status, errors = wc.tx_build_host(a, f_off, descs, socks, None, SLOT)
            ts_build.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            st2, err2 = wc.tx_seal_host(b, f_off, f_len)
            ts_seal.append(time.perf_counter() - t0)
        same = bool(np.array_equal(a, b))
        if registered:
            wc.host_unregister(a)
            wc.host_unregister(b)
        kind = "registered" if registered else "pageable"
        for name, ts in (("wc_tx_build_host", ts_build[1:]),
                         ("wc_tx_seal_host (headers already written)", ts_seal[1:])):
            print(f"host {kind:10s} {name:42s} best {nbytes / min(ts) / 1e9:6.1f} GB/s median "
                  f"{nbytes / statistics.median(ts) / 1e9:6.1f} GB/s, median "
                  f"{statistics.median(ts) * 1e3:.1f} ms ({len(ts)} calls of {n} frames)",
                  flush=True)
        print(f"host {kind}: {int((status == wc.TX_SEALED).sum())} SEALED, {errors} errors; "
              f"both buffers identical: {same}", flush=True)
        if not same or errors or err2 or not np.array_equal(flen, f_len):
            raise SystemExit("the built buffer and the sealed one differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=2)
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.host:
        host_calls(args)
    else:
        device_pairs(args)


if __name__ == "__main__":
    main()
