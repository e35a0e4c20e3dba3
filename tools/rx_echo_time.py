#!/usr/bin/env python3
"""wc_rx_echo timed: the three routes from a ring to a built TX batch, and copy
mode against a plain device copy.

(a) A 4096-frame ring in 2048-byte slots, frames to 16 sockets of which every
second one is echoed (8 on), from peers whose MACs the neighbour table holds;
two rings: `mtu` (1472-byte payloads) and `mixed` (the lengths of
tests/rx_echo_cases.LENS in turn).  m = n: the pump takes all 4096 entries, the
inert ones included.  Three routes, all through the C ABI on preallocated
outputs, each timed as the host's clock around its calls and one synchronize:

    in-place  wc_rx_drain -> wc_rx_echo (tx_off) -> wc_tx_pump on the RX buffer
    copy      wc_rx_drain -> wc_rx_echo (slots)  -> wc_tx_pump on the slots
    host      the only route without wc_rx_echo: wc_rx_drain, a synchronize, a
              readback of start / list / rec and of the first 64 bytes of every
              frame (MACs and addresses), numpy descriptors and destinations,
              their upload, a device gather of the payloads, wc_tx_pump.
              The gather is one torch.index_select of whole 2048-byte slots --
              possible only because these rings carry no IPv4 options, so a
              payload lies at the same offset in its RX slot and its TX slot; a
              ring with options needs a byte gather, which is not timed here.

The in-place pump rewrites the RX frames, so the RX buffer is restored from a
copy before every timed iteration of every route (not timed).  Before timing,
the built frames of the three routes are compared byte for byte.

(b) Copy mode alone over 65536 frames of 1472 payload bytes (one socket, all
echoed, m = 65536), timed with device events around the one launch, against a
device-to-device copy (hipMemcpyDtoD through torch's copy_) of the same payload
byte count, alternating in the same run.  The rate is over payload bytes read
plus payload bytes written, as a fraction of the HBM peak of 8 TB/s; the
metadata (some 64 bytes per frame) is not counted.  The ring and the slots are
128 MiB each: part of either may sit in the 256 MiB Infinity Cache, for the
copy as for the echo.

Each figure is the median of `--calls` (at least 200) after `--warmup`, with the
minimum and maximum.

    python tools/rx_echo_time.py [--calls 200] [--warmup 30]
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

import rx_demux_cases as dc  # noqa: E402
import rx_echo_cases as cases  # noqa: E402
import rx_reply_cases as rc  # noqa: E402
import tx_neigh_model as tmodel  # noqa: E402
import warpcore_amd as wc  # noqa: E402
from rx_drain import ring  # noqa: E402
from warpcore_amd import _lib  # noqa: E402
from warpcore_amd.cksum import _DrainOut, _EchoOut, _PumpOut  # noqa: E402

SLOT, HBM_PEAK = 2048, 8.0e12
PEERS = cases.PEERS4 + cases.PEERS6 + [dc.PEER4, dc.PEER6]


def dev_bytes(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def table(dev):
    """A neighbour table that holds every peer's MAC."""
    tab = wc.neigh_tab_init(64, dev)
    upd = tmodel.records([(4 if len(a) == 4 else 6, bytes((2, 9, 9, 9, 9, k)), a)
                          for k, a in enumerate(dict.fromkeys(PEERS))])
    wc.neigh_apply(tab, dev_bytes(upd, dev).reshape(-1, 24),
                   torch.tensor([len(upd)], dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    return tab


def stats(ts):
    return (f"{statistics.median(ts) * 1e6:8.1f} us ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})")


class Turn:
    """One ring, its sockets and every preallocated output of the three routes."""

    def __init__(self, dev, lib, socks, frames, n, emap):
        self.dev, self.lib, self.n, self.m = dev, lib, n, min(n, wc.RX_ECHO_MAX)
        m = self.m
        self.buf, self.d_off, self.d_len = ring(dev, frames, n)
        self.buf0 = self.buf.clone()
        self.ns = len(socks)
        self.d_tab = dev_bytes(wc.rx_socktab_build(socks), dev)
        self.d_eng = dev_bytes(rc.engine_table(), dev)
        self.d_socks = dev_bytes(cases.tx_socks(socks), dev)
        self.emap = np.asarray(emap, np.uint16)
        self.d_map = torch.from_numpy(self.emap.view(np.int16).copy()).to(dev)
        self.neigh = table(dev)
        self.plan = wc.rx_drain(self.buf, self.d_off, self.d_len, self.d_tab, self.ns, self.d_eng,
                                SLOT)
        self.drain_out = _DrainOut(*[t.data_ptr() for t in self.plan])
        self.drain_scratch = torch.zeros(wc.rx_drain_scratch(n) // 4 + 1, dtype=torch.int32,
                                         device=dev)
        z = lambda k, dt=torch.uint8: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
        self.slots = z(m * SLOT + 64)
        self.toff = torch.arange(m, dtype=torch.int64, device=dev) * SLOT
        # the echo's outputs (both modes share all but tx_off) and the host route's own
        self.e = {"desc": z(8 * m), "dsts": z(24 * m), "af": z(m), "status": z(m),
                  "src": z(m, torch.int32), "tx_off": z(m, torch.int64), "count": z(1, torch.int64),
                  "skipped": z(1, torch.int64)}
        self.h = {"desc": z(8 * m), "dsts": z(24 * m), "af": z(m), "idx": z(m, torch.int64)}
        p = {k: v.data_ptr() for k, v in self.e.items()}
        self.echo_out = {
            "copy": _EchoOut(p["desc"], p["dsts"], p["af"], p["status"], p["src"], None, p["count"],
                             p["skipped"]),
            "in-place": _EchoOut(p["desc"], p["dsts"], p["af"], p["status"], p["src"], p["tx_off"],
                                 p["count"], p["skipped"])}
        self.sol = z(m * 128)
        self.sol_off = torch.arange(m, dtype=torch.int64, device=dev) * 128
        self.pump = {k: [z(m), z(m, torch.int32), z(1, torch.int64), z(m), z(m, torch.int32),
                         z(1, torch.int64), z(m, torch.uint16), z(1, torch.int64),
                         z(m, torch.uint16), z(m), z(m, torch.uint16), z(m, torch.uint16),
                         z(1, torch.int64)] for k in ("in-place", "copy", "host")}
        self.pump_out = {k: _PumpOut(*[t.data_ptr() for t in v]) for k, v in self.pump.items()}
        self.pump_scratch = z(wc.tx_pump_scratch(m, m) // 4 + 1, torch.int32)
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def restore(self):
        self.buf.copy_(self.buf0)
        torch.cuda.synchronize()

    def drain(self):
        return self.lib.wc_rx_drain(self.buf.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(),
                                    self.n, self.d_tab.data_ptr(), self.ns, self.d_eng.data_ptr(),
                                    SLOT, ctypes.byref(self.drain_out),
                                    self.drain_scratch.data_ptr(), self.st)

    def echo(self, mode: str):
        copy = mode == "copy"
        pl = self.plan
        return self.lib.wc_rx_echo(self.buf.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(),
                                   self.n, pl.records.data_ptr(), pl.list.data_ptr(),
                                   pl.start.data_ptr(), self.d_map.data_ptr(), self.ns, None,
                                   self.slots.data_ptr() if copy else None,
                                   self.toff.data_ptr() if copy else None, SLOT, self.m,
                                   ctypes.byref(self.echo_out[mode]), self.st)

    def pump_call(self, route: str, src: dict, base, offs, slot: int):
        m = self.m
        return self.lib.wc_tx_pump(self.neigh.data_ptr(), src["dsts"].data_ptr(),
                                   src["af"].data_ptr(), m, src["desc"].data_ptr(), m,
                                   self.d_socks.data_ptr(), self.ns, base.data_ptr(), offs.data_ptr(),
                                   slot, 0, self.d_eng.data_ptr(), self.sol.data_ptr(),
                                   self.sol_off.data_ptr(), m, 128, ctypes.byref(self.pump_out[route]),
                                   self.pump_scratch.data_ptr(), self.st)

    def route(self, name: str) -> int:
        rc_ = self.drain()
        if name == "in-place":
            return rc_ or self.echo(name) or self.pump_call(name, self.e, self.buf, self.e["tx_off"],
                                                            SLOT - 40)
        if name == "copy":
            return rc_ or self.echo(name) or self.pump_call(name, self.e, self.slots, self.toff, SLOT)
        return rc_ or self.host_route()

    def host_route(self) -> int:
        n, m, pl = self.n, self.m, self.plan
        torch.cuda.synchronize()
        start = pl.start.cpu().numpy().view(np.uint64)
        lst = pl.list.cpu().numpy().view(np.uint32)
        rec = pl.records.cpu().numpy().reshape(-1).view(wc.RX_RECORD)
        hdr = self.buf[:n * SLOT].view(n, SLOT)[:, :64].cpu().numpy()
        on = [s for s in range(self.ns) if self.emap[s] <= 255 and start[s] <= start[s + 1] <= n]
        idx = np.concatenate([lst[int(start[s]):int(start[s + 1])] for s in on] or
                             [np.zeros(0, np.uint32)])[:m].astype(np.int64)
        sock = np.concatenate([np.full(int(start[s + 1] - start[s]), self.emap[s] & 0xFF, np.uint8)
                               for s in on] or [np.zeros(0, np.uint8)])[:m]
        E = len(idx)
        r, h = rec[idx], hdr[idx]
        desc = np.zeros(m, wc.TX_DESC)
        desc["data_len"], desc["dst"] = 0xFFFF, np.arange(m)
        desc["data_len"][:E], desc["sock"][:E], desc["tos"][:E] = r["data_len"], sock, r["tos"]
        dsts, af = np.zeros(m, wc.TX_DST), np.zeros(m, np.uint8)
        v4 = r["af"] == 4
        dsts["addr"][:E][v4, :4] = h[v4, 26:30]
        dsts["addr"][:E][~v4] = h[~v4, 22:38]
        dsts["dmac"][:E], dsts["port"][:E], af[:E] = h[:, 6:12], r["sport"], r["af"]
        rows = np.zeros(m, np.int64)
        rows[:E] = idx
        self.h["desc"].copy_(torch.from_numpy(desc.view(np.uint8).reshape(-1)))
        self.h["dsts"].copy_(torch.from_numpy(dsts.view(np.uint8).reshape(-1)))
        self.h["af"].copy_(torch.from_numpy(af))
        self.h["idx"].copy_(torch.from_numpy(rows))
        torch.index_select(self.buf[:n * SLOT].view(n, SLOT), 0, self.h["idx"],
                           out=self.slots[:m * SLOT].view(m, SLOT))
        return self.pump_call("host", self.h, self.slots, self.toff, SLOT)

    def built(self, route: str):
        """[frame bytes] of every built entry, after the route ran."""
        torch.cuda.synchronize()
        flen = self.pump[route][8].cpu().numpy()
        offs = (self.e["tx_off"] if route == "in-place" else self.toff).cpu().numpy()
        mem = (self.buf if route == "in-place" else self.slots).cpu().numpy()
        return [mem[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, flen)]


def part_a(dev, lib, args):
    socks = dc.population(16, 1)
    emap = cases.echo_map(16, "alternating")
    rng = np.random.default_rng(2)
    for name, lens in (("mtu", (1472,)), ("mixed", cases.LENS)):
        frames = [cases.sized_frame_to(rng, socks[k % 16], lens[(k // 16) % len(lens)], k)[0]
                  for k in range(16 * max(len(lens), 4))]
        t = Turn(dev, lib, socks, frames, 4096, emap)
        frames_of = {}
        for route in ("in-place", "copy", "host"):
            t.restore()
            if t.route(route):
                raise SystemExit(f"{route}: a call failed")
            frames_of[route] = t.built(route)
        E = int(t.e["count"].item())
        nb = sum(1 for f in frames_of["copy"] if f)
        same = frames_of["in-place"] == frames_of["copy"] == frames_of["host"]
        print(f"check, {name}: E = {E} of n = 4096, {nb} frames built, "
              f"{sum(map(len, frames_of['copy']))} bytes; the three routes build the same frames: "
              f"{same}", flush=True)
        if not same or nb != E:
            raise SystemExit("route check failed")
        ts = {k: [] for k in ("in-place", "copy", "host")}
        for i in range(args.warmup + args.calls):
            for route in ts:
                t.restore()
                t0 = time.perf_counter()
                t.route(route)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[route].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for route in ts:
            print(f"(a) {name:5s} {route:8s}: {stats(ts[route])} | host / this "
                  f"{med['host'] / med[route]:.2f}", flush=True)
        # the echo launch alone, by device events
        for mode in ("in-place", "copy"):
            ev = []
            for i in range(args.warmup + args.calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t.echo(mode)
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    ev.append(a.elapsed_time(b) * 1e-3)
            print(f"(a) {name:5s} wc_rx_echo alone, {mode:8s} (device events): {stats(ev)}",
                  flush=True)


def part_b(dev, lib, args):
    n = 65536
    socks = dc.population(1, 1)
    rng = np.random.default_rng(3)
    frames = [cases.sized_frame_to(rng, socks[0], 1472, k)[0] for k in range(64)]
    t = Turn(dev, lib, socks, frames, n, cases.echo_map(1, "all"))
    if t.echo("copy"):
        raise SystemExit("echo failed")
    torch.cuda.synchronize()
    E, status = int(t.e["count"].item()), t.e["status"].cpu().numpy()
    got = t.slots[:n * SLOT].view(n, SLOT)[:, 42:42 + 1472].cpu().numpy()
    want = t.buf0[:n * SLOT].view(n, SLOT)[:, 42:42 + 1472].cpu().numpy()
    ok = E == n and not status.any() and np.array_equal(got, want)
    print(f"check, 65536 x 1472: E = {E}, every status ECHO and every payload copied: {ok}",
          flush=True)
    if not ok:
        raise SystemExit("copy check failed")
    nbytes = n * 1472
    a_src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    a_dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ts = {"echo": [], "memcpy": []}
    for i in range(args.warmup + args.calls):
        for k in ts:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if k == "echo":
                t.echo("copy")
            else:
                a_dst.copy_(a_src)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ts[k].append(a.elapsed_time(b) * 1e-3)
    for k in ts:
        md = statistics.median(ts[k])
        rate = 2 * nbytes / md
        print(f"(b) {k:6s}: {stats(ts[k])} | {2 * nbytes / 1e6:.1f} MB read + written, "
              f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak",
              flush=True)
    print(f"(b) memcpy / echo: {statistics.median(ts['memcpy']) / statistics.median(ts['echo']):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    if args.calls < 200:
        raise SystemExit("--calls: at least 200")
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    lib = _lib.active()
    print(f"== wc_rx_echo: {args.calls} calls after {args.warmup}; slots of {SLOT} bytes; "
          f"{wc.version()}", flush=True)
    part_a(dev, lib, args)
    part_b(dev, lib, args)
    print("(not taken: rocprofv3 kernel times, rings with IPv4 options on the host route, m other "
          "than n, the pump's larger path above 4096 entries)")


if __name__ == "__main__":
    main()
