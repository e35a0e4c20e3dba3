#!/usr/bin/env python3
"""TX neighbours timed in one process, each call between two device events.

    apply      2^16 update records into a fresh 2^18-entry table: half of them
               new keys, half repeats of those keys with other MACs
    resolve    65536 destinations over that table, at hit rates 1.0 and 0.5 (the
               misses drawn from 4096 unknown addresses, so most are duplicates),
               with and without the solicit list
    hold plan  2^20 frames over four sockets and the 0.5 table's states
    solicit    2^15 ARP who-has frames, then 2^15 neighbour solicitations, into
               128-byte slots
    host       wc_neigh_tab_lookup for the same 65536 destinations over a host
               copy of the table, on one core, through ctypes -- beside the same
               number of calls of a function that does nothing, since the
               Python call dominates both

Before timing, every result is checked against a dict model built here: the
lookups of every key, all states, the destination MACs, the list, the hold
codes, every length and a sample of the frames.

    python tools/tx_neigh.py [--rounds 8] [--warmup 2]

For kernel times run the same command under `rocprofv3 --kernel-trace --stats`,
as a run of its own.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import warpcore_amd as wc  # noqa: E402
from rx_deliver import timed  # noqa: E402
from rx_reply import A4, A6, MAC, csum, engine  # noqa: E402

CAP, RECORDS, NDST, FRAMES, SOLICIT, SLOT = 1 << 18, 1 << 16, 1 << 16, 1 << 20, 1 << 15, 128
BCAST = b"\xff" * 6


def key_bytes(i: int):
    """Key i: af 4 for even i, af 6 for odd."""
    if i % 2 == 0:
        return 4, bytes((10, (i >> 16) & 0xFF, (i >> 8) & 0xFF, i & 0xFF)) + bytes(12)
    return 6, bytes.fromhex("20010db8") + bytes(8) + i.to_bytes(4, "big")


def records(rng):
    """RECORDS records: the first half new keys 0 .. RECORDS / 2, the second
    half repeats of random ones; and the dict they leave."""
    upd = np.zeros(RECORDS, wc.NEIGH_UPDATE)
    ids = np.concatenate([np.arange(RECORDS // 2), rng.integers(0, RECORDS // 2, RECORDS // 2)])
    upd["mac"] = rng.integers(0, 255, (RECORDS, 6), dtype=np.uint8)  # never ff x 6
    cache = {}
    for j, i in enumerate(ids.tolist()):
        af, a = key_bytes(i)
        upd["af"][j] = af
        upd["addr"][j] = np.frombuffer(a, np.uint8)
        cache[(af, a)] = bytes(upd["mac"][j])
    return upd, cache


def destinations(rng, hit: float):
    dsts = np.zeros(NDST, wc.TX_DST)
    afs = np.empty(NDST, np.uint8)
    known = rng.random(NDST) < hit
    ids = np.where(known, rng.integers(0, RECORDS // 2, NDST), (1 << 20) + rng.integers(0, 4096, NDST))
    for k, i in enumerate(ids.tolist()):
        afs[k], a = key_bytes(i)
        dsts["addr"][k] = np.frombuffer(a, np.uint8)
    dsts["port"] = 0x5111
    return dsts, afs


def model_resolve(cache, dsts, afs):
    state = np.zeros(NDST, np.uint8)
    mac = np.full((NDST, 6), 0xFF, np.uint8)
    seen = set()
    for k in range(NDST):
        key = (int(afs[k]), bytes(dsts["addr"][k]))
        m = cache.get(key)
        if m is not None:
            mac[k] = np.frombuffer(m, np.uint8)
        else:
            state[k] = wc.NR_MISS_DUP if key in seen else wc.NR_MISS
            seen.add(key)
    return state, mac


def who_has(tpa: bytes) -> bytes:
    return BCAST + MAC + b"\x08\x06\x00\x01\x08\x00\x06\x04\x00\x01" + MAC + A4 + bytes(6) + tpa


def nsol(tgt: bytes) -> bytes:
    m = b"\x87\x00\x00\x00\x60\x00\x00\x00" + tgt + b"\x01\x01" + MAC
    h = b"\x60\x00\x00\x00" + len(m).to_bytes(2, "big") + b"\x3a\xff" + A6 + \
        bytes.fromhex("ff0200000000000000000001ff") + tgt[13:]
    ck = csum(h[8:40] + h[4:6] + m, 58 << 24)
    return b"\x33\x33" + tgt[12:] + MAC + b"\x86\xdd" + h + m[:2] + ck + m[4:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    rng = np.random.default_rng(5)

    def dev_bytes(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    upd, cache = records(rng)
    d_upd = dev_bytes(upd).reshape(-1, 24)
    d_cnt = torch.tensor([RECORDS], dtype=torch.int64, device=dev)
    tab = wc.neigh_tab_init(CAP, dev)
    dropped = wc.neigh_apply(tab, d_upd, d_cnt)
    torch.cuda.synchronize()
    h_tab = tab.cpu().numpy()
    ok = int(dropped.item()) == 0 and wc.neigh_tab_stats(h_tab) == (CAP, len(cache))
    ok = ok and all(wc.neigh_tab_lookup(h_tab, af, a) == m for (af, a), m in cache.items())
    print(f"== apply: {RECORDS} records, {len(cache)} distinct keys into a {CAP}-entry table "
          f"({wc.neigh_tab_bytes(CAP)} bytes)", flush=True)
    print(f"check: no record dropped, {len(cache)} entries used, every key's lookup is its last "
          f"record's MAC: {ok}", flush=True)
    if not ok:
        raise SystemExit("apply check failed")

    sets = {}
    for hit in (1.0, 0.5):
        dsts, afs = destinations(rng, hit)
        want_state, want_mac = model_resolve(cache, dsts, afs)
        d_dsts, d_af = dev_bytes(dsts), torch.from_numpy(afs).to(dev)
        state, lst, cnt = wc.tx_resolve(tab, d_dsts, d_af)
        after = d_dsts.cpu().numpy().view(wc.TX_DST)
        n = int(cnt.item())
        ok = bool((state.cpu().numpy() == want_state).all()) and bool((after["dmac"] == want_mac).all()) \
            and bool((after["addr"] == dsts["addr"]).all()) and bool((after["port"] == dsts["port"]).all()) \
            and lst.cpu().numpy().view(np.uint32)[:n].tolist() == np.flatnonzero(
                want_state == wc.NR_MISS).tolist()
        print(f"check, hit rate {hit}: {int((want_state == wc.NR_READY).sum())} ready, {n} to solicit, "
              f"{int((want_state == wc.NR_MISS_DUP).sum())} duplicates; states, MACs, list equal the "
              f"model: {ok}", flush=True)
        if not ok:
            raise SystemExit("resolve check failed")
        sets[hit] = (dsts, afs, d_dsts, d_af, state)

    dsts, afs, d_dsts, d_af, d_state = sets[0.5]
    socks = np.zeros(4, wc.TX_SOCK)
    socks["af"], socks["flags"] = (4, 6, 4, 6), (0, 0, wc.TX_SOCK_CONNECTED, wc.TX_SOCK_CONNECTED)
    descs = np.zeros(FRAMES, wc.TX_DESC)
    descs["dst"] = rng.integers(0, NDST, FRAMES)
    descs["sock"] = np.where(rng.random(FRAMES) < 0.25, 2, 0) + (afs[descs["dst"]] == 6)
    d_descs, d_socks = dev_bytes(descs), dev_bytes(socks)
    hold, hl, hc = wc.tx_hold_plan(d_descs, d_socks, d_state, d_af)
    st = d_state.cpu().numpy()[descs["dst"]]
    want = np.where((descs["sock"] >= 2) | (st == wc.NR_READY), wc.TH_READY, wc.TH_HELD).astype(np.uint8)
    ok = bool((hold.cpu().numpy() == want).all()) and int(hc.item()) == int((want == wc.TH_HELD).sum())
    print(f"check, hold plan: {FRAMES} frames, {int(hc.item())} held; codes and count equal the "
          f"model: {ok}", flush=True)
    if not ok:
        raise SystemExit("hold plan check failed")

    eng = torch.from_numpy(engine().view(np.uint8)).to(dev)
    out = torch.empty(SOLICIT * SLOT + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(SOLICIT, dtype=torch.int64, device=dev) * SLOT
    s_cnt = torch.tensor([SOLICIT], dtype=torch.int64, device=dev)
    lists = {}
    for af, ln in ((4, 42), (6, 86)):
        idx = np.resize(np.flatnonzero(afs == af), SOLICIT).astype(np.uint32)  # (some twice)
        d_idx = torch.from_numpy(idx.view(np.int32).copy()).to(dev)
        olen, built = wc.tx_solicit_build(d_dsts, d_af, d_idx, s_cnt, eng, out, o_off, SLOT)
        h_out = out.cpu().numpy()
        ok = idx.size == SOLICIT and bool((olen.cpu().numpy() == ln).all()) and int(built.item()) == SOLICIT
        for j in range(0, SOLICIT, 509):
            a = bytes(dsts["addr"][idx[j]])
            fr = who_has(a[:4]) if af == 4 else nsol(a)
            ok = ok and h_out[j * SLOT:j * SLOT + ln].tobytes() == fr
        print(f"check, solicit af {af}: {SOLICIT} frames of {ln} bytes, a sample of them equal to the "
              f"frames built here: {ok}", flush=True)
        if not ok:
            raise SystemExit("solicit check failed")
        lists[af] = d_idx

    def t_apply():
        wc.neigh_tab_init(CAP, tab=tab)
        return timed(lambda: wc.neigh_apply(tab, d_upd, d_cnt))

    calls = {
        "tab_init": lambda: timed(lambda: wc.neigh_tab_init(CAP, tab=tab)),
        "apply": t_apply,
        "resolve_hit1.0": lambda: timed(lambda: wc.tx_resolve(tab, sets[1.0][2], sets[1.0][3], want_list=False)),
        "resolve_hit1.0_list": lambda: timed(lambda: wc.tx_resolve(tab, sets[1.0][2], sets[1.0][3])),
        "resolve_hit0.5": lambda: timed(lambda: wc.tx_resolve(tab, d_dsts, d_af, want_list=False)),
        "resolve_hit0.5_list": lambda: timed(lambda: wc.tx_resolve(tab, d_dsts, d_af)),
        "hold_plan": lambda: timed(lambda: wc.tx_hold_plan(d_descs, d_socks, d_state, d_af, want_list=False)),
        "hold_plan_list": lambda: timed(lambda: wc.tx_hold_plan(d_descs, d_socks, d_state, d_af)),
        "solicit_arp": lambda: timed(lambda: wc.tx_solicit_build(d_dsts, d_af, lists[4], s_cnt, eng, out,
                                                                 o_off, SLOT, check=False)),
        "solicit_nsol": lambda: timed(lambda: wc.tx_solicit_build(d_dsts, d_af, lists[6], s_cnt, eng, out,
                                                                  o_off, SLOT, check=False)),
    }
    ts = {k: [] for k in calls}
    for i in range(args.warmup + args.rounds):
        t = {k: fn() for k, fn in calls.items()}
        tag = "warm" if i < args.warmup else "round"
        print(f"{tag} {i:2d}: " + " | ".join(f"{k} {v * 1e6:.1f}" for k, v in t.items()) + " us", flush=True)
        if i >= args.warmup:
            for k in ts:
                ts[k].append(t[k])
    # the table as the applies above left it
    wc.neigh_tab_init(CAP, tab=tab)
    wc.neigh_apply(tab, d_upd, d_cnt)
    torch.cuda.synchronize()
    print(f"== medians over {args.rounds} rounds (min .. max), us: " + "; ".join(
        f"{k} {statistics.median(v) * 1e6:.1f} ({min(v) * 1e6:.1f} .. {max(v) * 1e6:.1f})"
        for k, v in ts.items()), flush=True)

    # the host lookup, one core, through ctypes
    from warpcore_amd import _lib
    lib = _lib.active()
    h32 = np.ascontiguousarray(tab.cpu().numpy().view(np.uint32))
    tp, mac = h32.ctypes.data, (np.zeros(8, np.uint8))
    addrs = np.ascontiguousarray(dsts["addr"])
    ap0, mp, af_l = addrs.ctypes.data, mac.ctypes.data, afs.tolist()
    host, empty = [], []
    for _ in range(max(args.rounds, 5)):
        t0 = time.perf_counter()
        hits = 0
        for k in range(NDST):
            hits += lib.wc_neigh_tab_lookup(tp, af_l[k], ap0 + 16 * k, mp)
        t1 = time.perf_counter()
        for k in range(NDST):
            lib.wc_neigh_tab_bytes(64)
        t2 = time.perf_counter()
        host.append(t1 - t0), empty.append(t2 - t1)
    ok = hits == int((sets[0.5][4].cpu().numpy() == wc.NR_READY).sum())
    print(f"== host: {NDST} wc_neigh_tab_lookup calls {statistics.median(host) * 1e3:.1f} ms "
          f"({statistics.median(host) / NDST * 1e9:.0f} ns per call), {NDST} calls of a function that "
          f"does nothing {statistics.median(empty) * 1e3:.1f} ms "
          f"({statistics.median(empty) / NDST * 1e9:.0f} ns per call); hits equal the device's: {ok}")
    print("(device-event times of single calls, Python wrappers and their allocations included; "
          "kernel times: rocprofv3 --kernel-trace --stats)")


if __name__ == "__main__":
    main()
