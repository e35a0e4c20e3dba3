#!/usr/bin/env python3
"""wc_tx_pump timed against the chain it stands for, in one process and from the
same build (the chain's calls are unchanged code).

For n = 64, 256, 1024 and 4096 frames to ndst = n / 4 destinations, and for
4096 frames to 4096 destinations -- both thresholds at once -- (both
families, unconnected sockets, every frame's destination of its socket's
family), at neighbour-cache hit rates 1.0 and 0.5, in 2048-byte slots:

    mtu     1472-byte payloads
    mixed   payloads of 0 .. 1472 bytes

three paths are called through the C ABI on preallocated outputs (no Python
wrapper inside the timed region):

    (a) pump      wc_tx_pump                                       2 launches
    (b) honest    wc_tx_resolve, wc_tx_hold_plan, wc_tx_solicit_build with
                  their lists, then a D2H copy of d_hold, the READY frames'
                  offsets and descriptors compacted on the host and uploaded,
                  wc_tx_build_ragged on them: what a caller must do today.  The
                  staging buffers (pinned host, device) are allocated once,
                  outside the timed region; the compaction is numpy's
    (c) ungated   the same three calls, then wc_tx_build_ragged on EVERY frame
                  and no readback: the cheapest thing that can be written today;
                  its frame outputs are not the contract's (HELD frames get
                  ff:ff:ff:ff:ff:ff headers and a length)

Each timing is the host's clock around one path and one synchronize; the figure
is the median of `--calls` (at least 200) after `--warmup`, with the minimum and
maximum.  Before timing, every output of (a) is compared with (b)'s (scattered
back on the host) and the chain part of (c)'s.

    python tools/tx_pump.py [--calls 300] [--warmup 50] [--sizes 64,256,1024,4096]
                            [--extra 4096:4096]
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

import rx_reply_cases as rc  # noqa: E402
import tx_neigh_cases as nc  # noqa: E402
import tx_neigh_model as nmodel  # noqa: E402
import warpcore_amd as wc  # noqa: E402
from warpcore_amd import _lib  # noqa: E402
from warpcore_amd.cksum import _PumpOut  # noqa: E402

SLOT, SOL_SLOT = 2048, 128
MEMBERS = [name for name, _ in _PumpOut._fields_]


def dev_bytes(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


class Path_:
    """One path's own tensors: the three it writes into and the thirteen outputs."""

    def __init__(self, dev, n, ndst, m, dsts, frames, sol):
        self.dsts, self.buf, self.sol = dev_bytes(dsts, dev), frames.clone(), sol.clone()
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
        self.t = dict(state=z(ndst, torch.uint8), miss_list=z(ndst, torch.int32),
                      miss_count=z(1, torch.int64), hold=z(n, torch.uint8), held_list=z(n, torch.int32),
                      held_count=z(1, torch.int64), sol_len=z(m, torch.uint16), sol_built=z(1, torch.int64),
                      frame_len=z(n, torch.uint16), status=z(n, torch.uint8), out_ip_hdr=z(n, torch.uint16),
                      out_udp=z(n, torch.uint16), errors=z(1, torch.int64))
        self.p = {k: v.data_ptr() for k, v in self.t.items()}
        self.c = _PumpOut(*[self.p[k] for k in MEMBERS])

    def host(self, frames: bool = True):
        h = {k: v.cpu().numpy() for k, v in self.t.items() if k != "errors"}
        for lst, cnt in (("miss_list", "miss_count"), ("held_list", "held_count")):
            h[lst] = h[lst][:int(h[cnt][0])]
        h["dsts"], h["sol"] = self.dsts.cpu().numpy(), self.sol.cpu().numpy()
        if frames:
            h["buf"] = self.buf.cpu().numpy()
        else:
            for k in ("frame_len", "status", "out_ip_hdr", "out_udp"):
                del h[k]
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--extra", default="4096:4096", help="further n:ndst pairs")
    args = ap.parse_args()
    if args.calls < 200:
        raise SystemExit("--calls: at least 200")
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    lib = _lib.active()
    st = torch.cuda.current_stream(dev).cuda_stream
    socks = nc.socks_table()[:2]
    d_socks, ns = dev_bytes(socks, dev), 2
    d_eng = dev_bytes(rc.engine_table(), dev)
    print(f"== wc_tx_pump against the chain: {args.calls} calls after {args.warmup}, one synchronize "
          f"per call; ndst = n / 4 and {args.extra}, m = ndst, slot_bytes {SLOT}; WC_TX_PUMP_SMALL = {wc.TX_PUMP_SMALL}, "
          f"WC_TX_PUMP_SMALL_DST = {wc.TX_PUMP_SMALL_DST}", flush=True)
    pairs = [(n, n // 4) for n in (int(x) for x in args.sizes.split(","))]
    pairs += [(int(n), int(d)) for n, d in (p.split(":") for p in args.extra.split(",") if p)]
    for batch in ("mtu", "mixed"):
        for hit in (1.0, 0.5):
            for n, ndst in pairs:
                rng = np.random.default_rng(n + ndst)
                m = ndst
                ks = nc.keys(ndst)
                nknown = int(round(hit * ndst))
                known = [ks[i] for i in rng.permutation(ndst)[:nknown]]
                tab = wc.neigh_tab_init(max(64, 1 << (4 * ndst).bit_length()), dev)
                if known:
                    upd = nmodel.records([(af, nc.mac_of(rng), a) for af, a in known])
                    wc.neigh_apply(tab, dev_bytes(upd, dev).reshape(-1, 24),
                                   torch.tensor([upd.size], dtype=torch.int64, device=dev))
                dsts = nc.dst_table([(a, 4433) for _, a in ks], rng)
                afs = np.array([af for af, _ in ks], np.uint8)
                descs = np.zeros(n, nmodel.DESC)
                descs["dst"] = rng.integers(0, ndst, n)
                descs["sock"] = np.where(afs[descs["dst"]] == 4, 0, 1)
                descs["data_len"] = 1472 if batch == "mtu" else rng.integers(0, 1473, n)
                descs["ip_id"] = rng.integers(0, 65536, n)
                offs = np.arange(n, dtype=np.uint64) * SLOT
                frames = torch.from_numpy(rng.integers(0, 256, n * SLOT + 64, dtype=np.uint8)).to(dev)
                sol0, sol_offs = rc.out_slots(m, SOL_SLOT, rng)
                sol = torch.from_numpy(sol0).to(dev)
                d_af, d_descs = torch.from_numpy(afs).to(dev), dev_bytes(descs, dev)
                d_offs, d_sol_offs = torch.from_numpy(offs).to(dev), torch.from_numpy(sol_offs).to(dev)
                A, B, C = (Path_(dev, n, ndst, m, dsts, frames, sol) for _ in range(3))
                scratch = torch.zeros(wc.tx_pump_scratch(n, ndst) // 4 + 1, dtype=torch.int32, device=dev)
                tp, ap_, dp, sp, op, ep, so, sc = (tab.data_ptr(), d_af.data_ptr(), d_descs.data_ptr(),
                                                   d_socks.data_ptr(), d_offs.data_ptr(), d_eng.data_ptr(),
                                                   d_sol_offs.data_ptr(), scratch.data_ptr())

                def pump():
                    return lib.wc_tx_pump(tp, A.dsts.data_ptr(), ap_, ndst, dp, n, sp, ns, A.buf.data_ptr(),
                                          op, SLOT, 0, ep, A.sol.data_ptr(), so, m, SOL_SLOT,
                                          ctypes.byref(A.c), sc, st)

                def plan(X):
                    p, dd = X.p, X.dsts.data_ptr()
                    return (lib.wc_tx_resolve(tp, dd, ap_, ndst, p["state"], p["miss_list"],
                                              p["miss_count"], sc, st)
                            or lib.wc_tx_hold_plan(dp, n, sp, ns, p["state"], ap_, ndst, p["hold"],
                                                   p["held_list"], p["held_count"], sc, st)
                            or lib.wc_tx_solicit_build(dd, ap_, ndst, p["miss_list"], p["miss_count"], ep,
                                                       X.sol.data_ptr(), so, m, SOL_SLOT, p["sol_len"],
                                                       p["sol_built"], st))

                bt = dict(frame_len=torch.zeros(n, dtype=torch.uint16, device=dev),
                          status=torch.zeros(n, dtype=torch.uint8, device=dev),
                          out_ip_hdr=torch.zeros(n, dtype=torch.uint16, device=dev),
                          out_udp=torch.zeros(n, dtype=torch.uint16, device=dev))
                ready = [None]
                # (b)'s staging, allocated once: pinned host buffers for the readback and
                # the compacted arrays, device buffers for their upload
                hold_h = torch.empty(n, dtype=torch.uint8).pin_memory()
                off_h = torch.empty(n, dtype=torch.int64).pin_memory()
                desc_h = torch.empty((n, 8), dtype=torch.uint8).pin_memory()
                off_c = torch.empty(n, dtype=torch.int64, device=dev)
                desc_c = torch.empty((n, 8), dtype=torch.uint8, device=dev)
                offs_i, descs_b = offs.view(np.int64), descs.view(np.uint8).reshape(n, 8)

                def honest():
                    if plan(B):
                        return 1
                    hold_h.copy_(B.t["hold"][:n])  # the readback, a synchronize
                    idx = np.flatnonzero(hold_h.numpy() == wc.TH_READY)
                    ready[0] = idx
                    k = idx.size
                    if k == 0:
                        return 0
                    off_h.numpy()[:k] = offs_i[idx]
                    desc_h.numpy()[:k] = descs_b[idx]
                    off_c[:k].copy_(off_h[:k], non_blocking=True)
                    desc_c[:k].copy_(desc_h[:k], non_blocking=True)
                    return lib.wc_tx_build_ragged(B.buf.data_ptr(), off_c.data_ptr(), desc_c.data_ptr(),
                                                  k, sp, ns, B.dsts.data_ptr(), ndst, SLOT, 0,
                                                  bt["frame_len"].data_ptr(), bt["status"].data_ptr(),
                                                  bt["out_ip_hdr"].data_ptr(), bt["out_udp"].data_ptr(),
                                                  B.p["errors"], st)

                def ungated():
                    p = C.p
                    return plan(C) or lib.wc_tx_build_ragged(
                        C.buf.data_ptr(), op, dp, n, sp, ns, C.dsts.data_ptr(), ndst, SLOT, 0,
                        p["frame_len"], p["status"], p["out_ip_hdr"], p["out_udp"], p["errors"], st)

                if pump() or honest() or ungated():
                    raise SystemExit("a call failed")
                torch.cuda.synchronize()
                ha, hb, hc = A.host(), B.host(), C.host(frames=False)
                idx = ready[0]
                hb["status"] = np.where(hb["hold"][:n] == wc.TH_HELD, wc.TX_PUMP_HELD,
                                        wc.TX_MALFORMED).astype(np.uint8)
                for k in ("frame_len", "out_ip_hdr", "out_udp"):
                    hb[k] = np.zeros(n, np.uint16)
                for k in bt:
                    hb[k][idx] = bt[k].cpu().numpy()[:idx.size]
                same_b = all(np.array_equal(ha[k][:len(hb[k])], hb[k]) for k in hb)
                same_c = all(np.array_equal(ha[k], hc[k]) for k in hc)
                held = int(ha["held_count"][0])
                print(f"check, {batch} hit {hit} n = {n}: pump == honest chain: {same_b}; pump's plan == "
                      f"ungated chain's: {same_c} ({int(ha['miss_count'][0])} misses, "
                      f"{int(ha['sol_built'][0])} solicitations, {held} held, {idx.size} built; the ungated "
                      f"build wrote {held} frames it must not)", flush=True)
                if not (same_b and same_c):
                    raise SystemExit("pump check failed")
                paths = (("pump", pump), ("honest", honest), ("ungated", ungated))
                ts = {k: [] for k, _ in paths}
                for i in range(args.warmup + args.calls):
                    for k, f in paths:
                        t0 = time.perf_counter()
                        f()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            ts[k].append(time.perf_counter() - t0)
                med = {k: statistics.median(v) for k, v in ts.items()}
                line = " | ".join(f"{k} {med[k] * 1e6:7.1f} us ({min(ts[k]) * 1e6:.1f} .. {max(ts[k]) * 1e6:.1f})"
                                  for k, _ in paths)
                print(f"{batch:5s} hit {hit} n = {n:4d} ndst = {ndst:4d}: {line} | honest / pump "
                      f"{med['honest'] / med['pump']:.2f} | ungated / pump {med['ungated'] / med['pump']:.2f}",
                      flush=True)
    print("(host clock around one path and one synchronize, all paths through the C ABI on "
          "preallocated outputs)")


if __name__ == "__main__":
    main()
