#!/usr/bin/env python3
"""The TX seal timed beside the RX verdict on the same MTU netmap ring.

The ring is synth.make_rx_ring's: 2^20 well-formed UDP frames (2:1 IPv4 /
IPv6) of 1514 B in 2048-B slots, device-resident, `--rings` distinct buffers
(each 2 GiB, far past the 256 MiB Infinity Cache) taken in rotation.  Both
checksum fields of every frame are first overwritten with garbage.  In one
process, wc_tx_seal_ragged and wc_rx_verdict_ragged then alternate over the
rings, each call between two device events; per call the frame bytes over
the event time.  After the first seal of each ring every RX verdict must be
OK or OK_NO_CKSUM (the sealed-ring check).

    python tools/tx_seal.py [--pairs 8] [--warmup 2] [--rings 2] [--packets N]
    python tools/tx_seal.py --host [--reps 3]

--host: the host calls over the e2e leg's 2^20 MTU frames in host memory,
registered and pageable: wc_tx_seal_host against wc_cksum_ip_udp_host plus a
store pass (numpy's vectorised scatter here, where an integrator has a C
loop), wall-clock per call.

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
from warpcore_amd import _lib, synth  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes / s


def build_ring(dev, n, seed, slot=2048, ip_len=1500):
    buf = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    wc.synth_fill(buf, seed, nbytes=n * slot)
    f_off, f_len = synth.make_rx_ring(buf, n, np.full(n, ip_len, dtype=np.uint16), slot=slot)
    # garbage in both fields: 0x0000, 0xFFFF or the slot's own random bytes
    ip = torch.from_numpy(f_off.astype(np.int64)).to(dev) + 14
    v6 = (torch.arange(n, device=dev) % 3) == 0  # make_rx_ring's v6_every
    k = torch.arange(n, device=dev) % 4
    fill = torch.where(k == 0, 0x00, 0xFF).to(torch.uint8)
    junk = buf[ip + 60]
    val = torch.where(k < 2, fill, junk)
    o4 = ip[~v6]
    buf[o4 + 10] = val[~v6]
    buf[o4 + 11] = val[~v6]
    ucs = ip + torch.where(v6, 46, 26)
    buf[ucs] = val
    buf[ucs + 1] = val
    return buf, f_off, f_len


def device_pairs(args):
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    n = args.packets
    rings = [build_ring(dev, n, 11 + 7 * r) for r in range(args.rings)]
    f_off, f_len = rings[0][1], rings[0][2]
    d_off = torch.from_numpy(f_off).to(dev)
    d_len = torch.from_numpy(f_len).to(dev)
    nbytes = int(f_len.astype(np.uint64).sum())
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    drops = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    errors = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = _lib.active()
    stream = torch.cuda.current_stream().cuda_stream

    def seal(buf):  # the C call itself: nothing allocated between the events
        rc = lib.wc_tx_seal_ragged(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, 0,
                                   status.data_ptr(), None, None, errors.data_ptr(), stream)
        if rc:
            raise SystemExit(f"wc_tx_seal_ragged: {rc}")

    print(f"ring: {n} frames of {nbytes / n:.0f} B in 2048-B slots, {args.rings} buffers "
          f"of {n * 2048 / 2**30:.1f} GiB", flush=True)

    # the sealed-ring check, on every buffer's first seal
    for r, (buf, _, _) in enumerate(rings):
        st, _, _, errs = wc.tx_seal_ragged(buf, d_off, d_len, check=r == 0)
        v, _ = wc.rx_verdict_ragged(buf, d_off, d_len, check=False)
        sealed = int((st == wc.TX_SEALED).sum())
        ok = int(((v == wc.RX_OK) | (v == wc.RX_OK_NO_CKSUM)).sum())
        print(f"sealed-ring check, buffer {r}: {sealed} of {n} SEALED, {int(errs.item())} "
              f"errors; RX verdicts OK or OK_NO_CKSUM: {ok} of {n}", flush=True)
        if sealed != n or ok != n:
            raise SystemExit("sealed-ring check failed")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    seal_t, rx_t = [], []
    for i in range(args.warmup + args.pairs):
        buf = rings[i % args.rings][0]
        ts = timed(lambda: seal(buf))
        tr = timed(lambda: wc.rx_verdict_ragged(buf, d_off, d_len, out=out, check=False,
                                                drops=drops))
        tag = "warm" if i < args.warmup else "pair"
        print(f"{tag} {i:2d}: seal {ts * 1e6:8.1f} us {nbytes / ts / 1e12:6.3f} TB/s "
              f"({nbytes / ts / PEAK:.3f} of peak) | rx {tr * 1e6:8.1f} us "
              f"{nbytes / tr / 1e12:6.3f} TB/s ({nbytes / tr / PEAK:.3f} of peak)", flush=True)
        if i >= args.warmup:
            seal_t.append(ts)
            rx_t.append(tr)
    for name, ts in (("wc_tx_seal_ragged", seal_t), ("wc_rx_verdict_ragged", rx_t)):
        rate = [nbytes / t / PEAK for t in ts]
        print(f"== {name}: median {statistics.median(rate):.3f} of peak "
              f"(min {min(rate):.3f}, max {max(rate):.3f}) over {len(ts)} calls, "
              f"median {statistics.median(ts) * 1e6:.1f} us", flush=True)
    print("(device-event times of single calls; kernel times: rocprofv3 --kernel-trace --stats)")


def host_calls(args):
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    n, slot = args.packets, 2048
    buf, f_off, f_len = build_ring(dev, n, 23, slot=slot, ip_len=1472)
    garbled = buf.cpu().numpy()
    del buf
    nbytes = int(f_len.astype(np.uint64).sum())
    ip_off = f_off + np.uint64(14)
    ip_len = (f_len.astype(np.int64) - 14).astype(np.uint16)
    v6 = (np.arange(n) % 3) == 0
    ipo = ip_off.astype(np.int64)
    ucs = ipo + np.where(v6, 46, 26)

    def zero_fields(b):
        for at in (ipo[~v6] + 10, ipo[~v6] + 11, ucs, ucs + 1):
            b[at] = 0

    def pair_and_store(b):
        hdr, pay = wc.cksum_ip_udp_host(b, ip_off, ip_len)
        b[ipo[~v6] + 10] = (hdr[~v6] & 0xFF).astype(np.uint8)
        b[ipo[~v6] + 11] = (hdr[~v6] >> 8).astype(np.uint8)
        b[ucs] = (pay & 0xFF).astype(np.uint8)
        b[ucs + 1] = (pay >> 8).astype(np.uint8)

    for registered in (True, False):
        a, b = garbled.copy(), garbled.copy()
        zero_fields(b)  # the pair call needs both fields 0 in the bytes
        if registered:
            wc.host_register(a)
            wc.host_register(b)
        ts_seal, ts_pair = [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            status, errors = wc.tx_seal_host(a, f_off, f_len)
            ts_seal.append(time.perf_counter() - t0)
            zero_fields(b)
            t0 = time.perf_counter()
            pair_and_store(b)
            ts_pair.append(time.perf_counter() - t0)
        same = bool(np.array_equal(a, b))
        if registered:
            wc.host_unregister(a)
            wc.host_unregister(b)
        kind = "registered" if registered else "pageable"
        for name, ts in (("wc_tx_seal_host", ts_seal[1:]),
                         ("wc_cksum_ip_udp_host + store pass", ts_pair[1:])):
            print(f"host {kind:10s} {name:34s} best {nbytes / min(ts) / 1e9:6.1f} GB/s median "
                  f"{nbytes / statistics.median(ts) / 1e9:6.1f} GB/s ({len(ts)} calls of {n} "
                  f"frames)", flush=True)
        print(f"host {kind}: {int((status == wc.TX_SEALED).sum())} SEALED, {errors} errors; "
              f"both buffers identical: {same}", flush=True)
        if not same or errors:
            raise SystemExit("the sealed buffer and the pair call's differ")


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
