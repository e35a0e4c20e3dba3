#!/usr/bin/env python3
"""wc_rx_answer timed against the chain it stands for, in one process and from
the same build (the chain is unchanged code).

Rings in 2048-byte slots, planned once by wc_rx_drain; each list's m is its
count:

    mixed     the world of tests/rx_answer_cases.py (ARP and neighbour discovery
              with repeated addresses, ICMP of both families, UDP), 600
              host-built frames tiled to n = 64, 256, 1024 and 4096
    echo      4096 echo requests of 56 data bytes (every one a reply)
    echo-mtu  4096 echo requests of 1400 data bytes
    arp       1024 and 4096 ARP requests for our addresses from 64 hosts (every
              one an is-at reply and an update record; with the table given,
              4096 records are above WC_RX_ANSWER_SMALL_APPLY: the chain's calls)

both paths are called through the C ABI on preallocated outputs (no Python
wrapper, no allocation inside the timed region), with the neighbour table given
and with tab NULL:

    answer  wc_rx_answer                                        2 launches
    chain   wc_rx_reply_build, wc_rx_neigh_updates, wc_rx_neigh_build
            [, wc_neigh_apply]             3 [+ 2] launches and 2 memsets

Each timing is the host's clock around one call (the chain: its three or four)
and one synchronize; the figure is the median of `--calls` (at least 200) after
`--warmup`, with the minimum and maximum.  Before timing, every output of the
answer is compared with the chain's, the tables through lookups of every
record's address.

    python tools/rx_answer.py [--calls 300] [--warmup 50] [--sizes 64,256,1024,4096]
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

import rx_answer_cases as cases  # noqa: E402
import rx_neigh_cases as nc  # noqa: E402
import rx_reply_cases as rc  # noqa: E402
import warpcore_amd as wc  # noqa: E402
from rx_drain import ring  # noqa: E402
from warpcore_amd import _lib  # noqa: E402
from warpcore_amd.cksum import _AnswerIo  # noqa: E402

SLOT, CAP = 2048, 4096


class Outputs:
    """One set of the answer's outputs, its slots, table and scratch."""

    def __init__(self, dev, ms):
        r_m, n_m, u_m = ms
        z = lambda k, dt=torch.uint8: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
        self.t = {"r_out": z(r_m * SLOT), "n_out": z(n_m * SLOT), "r_len": z(r_m, torch.uint16),
                  "n_len": z(n_m, torch.uint16), "r_built": z(1, torch.int64),
                  "n_built": z(1, torch.int64), "upd": z(24 * u_m), "dropped": z(1, torch.int64),
                  "scratch": z(wc.rx_answer_scratch(u_m) // 4 + 1, torch.int32)}
        self.tab = wc.neigh_tab_init(CAP, dev)
        self.p = {k: v.data_ptr() for k, v in self.t.items()}

    def host(self):
        h = {k: self.t[k].cpu().numpy() for k in self.t if k != "scratch"}
        tab = self.tab.cpu().numpy()
        u = h["upd"][:len(h["upd"]) // 24 * 24].view(wc.NEIGH_UPDATE)
        h["table"] = np.array([wc.neigh_tab_lookup(tab, int(r["af"]),
                                                   bytes(r["addr"][:4 if int(r["af"]) == 4 else 16]))
                               or b"" for r in u if int(r["af"]) in (4, 6)], dtype=object)
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
    seed, _, ns, _ = cases.WORLDS["slots"]
    frames, socks = cases.world(seed, 600, ns)
    rng = np.random.default_rng(seed)
    hosts = [(bytes((2, 0, 0, 5, 0, k)), bytes((192, 168, 90, 1 + k))) for k in range(64)]
    rings = [("mixed", frames, n) for n in (int(x) for x in args.sizes.split(","))]
    rings += [("echo", [rc.echo4(rng.integers(0, 256, 56, dtype=np.uint8).tobytes())
                        for _ in range(64)], 4096),
              ("echo-mtu", [rc.echo4(rng.integers(0, 256, 1400, dtype=np.uint8).tobytes())
                            for _ in range(64)], 4096),
              ("arp", [nc.arp(tpa=nc.A4[k % 2], sha=mac, spa=a) for k, (mac, a) in enumerate(hosts)],
               1024),
              ("arp", [nc.arp(tpa=nc.A4[k % 2], sha=mac, spa=a) for k, (mac, a) in enumerate(hosts)],
               4096)]
    d_tab = torch.from_numpy(wc.rx_socktab_build(socks).view(np.uint8).copy()).to(dev)
    d_eng = torch.from_numpy(rc.engine_table().view(np.uint8).reshape(-1).copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    print(f"== wc_rx_answer against its chain: {args.calls} calls after {args.warmup}, one "
          f"synchronize per call; slot_bytes {SLOT}, table cap {CAP}; WC_RX_ANSWER_SMALL = "
          f"{wc.RX_ANSWER_SMALL}, WC_RX_ANSWER_SMALL_APPLY = {wc.RX_ANSWER_SMALL_APPLY}", flush=True)
    for name, base, n in rings:
        buf, d_off, d_len = ring(dev, base, n)
        plan = wc.rx_drain(buf, d_off, d_len, d_tab, ns, d_eng, SLOT)
        torch.cuda.synchronize()
        ms = tuple(int(c.item()) for c in (plan.reply_count, plan.neigh_reply_count,
                                           plan.update_count))
        a, b = Outputs(dev, ms), Outputs(dev, ms)
        r_off = torch.arange(max(ms[0], 1), dtype=torch.int64, device=dev) * SLOT
        n_off = torch.arange(max(ms[1], 1), dtype=torch.int64, device=dev) * SLOT
        bp, op, lp, ep = buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_eng.data_ptr()
        pl = {k: getattr(plan, k).data_ptr() for k in plan._fields}
        rop, nop = r_off.data_ptr(), n_off.data_ptr()

        def io_of(o, tab):
            p = o.p
            return _AnswerIo(pl["actions"], pl["reply_list"], pl["reply_count"], pl["nact"],
                             pl["neigh_reply_list"], pl["neigh_reply_count"], pl["update_list"],
                             pl["update_count"], p["r_out"], rop, ms[0], None, p["r_len"],
                             p["r_built"], p["n_out"], nop, ms[1], p["n_len"], p["n_built"], ms[2],
                             p["upd"], o.tab.data_ptr() if tab else None, p["dropped"])

        ios = {True: io_of(a, True), False: io_of(a, False)}

        def answer(tab):
            return lib.wc_rx_answer(bp, op, lp, n, ep, SLOT, ctypes.byref(ios[tab]), a.p["scratch"], st)

        def chain(tab):
            p = b.p
            return (lib.wc_rx_reply_build(bp, op, lp, n, pl["actions"], pl["reply_list"],
                                          pl["reply_count"], ep, p["r_out"], rop, ms[0], SLOT, None,
                                          p["r_len"], p["r_built"], st)
                    or lib.wc_rx_neigh_updates(bp, op, lp, n, pl["nact"], pl["update_list"],
                                               pl["update_count"], ms[2], p["upd"], st)
                    or lib.wc_rx_neigh_build(bp, op, lp, n, pl["nact"], pl["neigh_reply_list"],
                                             pl["neigh_reply_count"], ep, p["n_out"], nop, ms[1], SLOT,
                                             p["n_len"], p["n_built"], st)
                    or (tab and ms[2] and lib.wc_neigh_apply(b.tab.data_ptr(), p["upd"],
                                                             pl["update_count"], ms[2], p["dropped"],
                                                             p["scratch"], st)) or 0)

        if answer(True) or chain(True):
            raise SystemExit("a call failed")
        torch.cuda.synchronize()
        ha, hb = a.host(), b.host()
        same = all(np.array_equal(ha[k], hb[k]) for k in ha)
        print(f"check, {name} n = {n}: every output of the answer equals the chain's: {same} "
              f"(r_m {ms[0]}, n_m {ms[1]}, u_m {ms[2]}; built {int(hb['r_built'][0])} + "
              f"{int(hb['n_built'][0])}, {len(hb['table'])} lookups)", flush=True)
        if not same:
            raise SystemExit("answer check failed")
        for tab in (True, False):
            ts = {"answer": [], "chain": []}
            for i in range(args.warmup + args.calls):
                for k, f in (("answer", answer), ("chain", chain)):
                    t0 = time.perf_counter()
                    f(tab)
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        ts[k].append(time.perf_counter() - t0)
            md, mc = statistics.median(ts["answer"]), statistics.median(ts["chain"])
            print(f"{name:8s} n = {n:4d} {'tab ' if tab else 'NULL'}: answer {md * 1e6:7.1f} us "
                  f"({min(ts['answer']) * 1e6:.1f} .. {max(ts['answer']) * 1e6:.1f}) | chain "
                  f"{mc * 1e6:7.1f} us ({min(ts['chain']) * 1e6:.1f} .. "
                  f"{max(ts['chain']) * 1e6:.1f}) | chain / answer {mc / md:.2f}", flush=True)
    print("(host clock around one call and one synchronize, both paths through the C ABI on "
          "preallocated outputs; not taken: the split between the two launches and the "
          "synchronize, rocprofv3 kernel times, anything above 4096)")


if __name__ == "__main__":
    main()
