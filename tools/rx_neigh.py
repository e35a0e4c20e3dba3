#!/usr/bin/env python3
"""RX neighbours timed beside the RX reply plan in front of them, in one process.

A ring of `--frames` Ethernet frames in 2048-byte slots (`--rings` distinct
device buffers taken in rotation) is tiled from 1024 host-built templates:

    mixed   every third frame a real ARP frame -- one request in eight for us,
            the others for other hosts, one in eight a reply to us -- the rest
            UDP datagrams of 0..1472 bytes for the one bound port
    arp     a flood of 60-byte ARP requests for us
    nsol    a flood of 86-byte neighbour solicitations for us

These calls alternate, each between two device events:

    wc_rx_reply_plan without its list      k_rx_reply_plan, the kernel in front
    wc_rx_neigh_plan without lists         k_rx_neigh_plan
    wc_rx_neigh_plan with both lists       seven launches
    wc_rx_neigh_updates                    one launch
    wc_rx_neigh_build                      one launch

Before timing, the device's codes, both counts, the built count and the records'
families are checked against the classes the ring was built from.

    python tools/rx_neigh.py [--ring mixed] [--frames 262144] [--rounds 8] [--warmup 2] [--rings 2]

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
from rx_reply import A4, A6, MAC, PEER6, PEER_MAC, SLOT, TEMPLATES, csum, engine, template  # noqa: E402

BCAST = b"\xff" * 6
CODE = {"udp": wc.RN_NONE, "arp_us": wc.RN_ARP_IS_AT, "arp_other": wc.RN_UPDATE4,
        "arp_reply": wc.RN_UPDATE4, "nsol": wc.RN_NADV}


def arp(op: int, tpa: bytes, rng, dst: bytes = BCAST) -> bytes:
    sha = bytes((2, 0, 0, 0, 1, int(rng.integers(0, 256))))
    spa = bytes((192, 168, int(rng.integers(0, 256)), int(rng.integers(1, 255))))
    tha = MAC if op == 2 else bytes(6)
    return dst + sha + b"\x08\x06\x00\x01\x08\x00\x06\x04\x00" + bytes((op,)) + sha + spa + tha + \
        tpa + bytes(18)


def nsol(rng) -> bytes:
    """A unicast solicitation (the table of rx_reply.engine() carries no snma)."""
    src = PEER6[:8] + rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
    m = b"\x87\x00\x00\x00" + bytes(4) + A6 + b"\x01\x01" + PEER_MAC
    h = b"\x60\x00\x00\x00" + len(m).to_bytes(2, "big") + b"\x3a\xff" + src + A6
    ck = csum(h[8:40] + h[4:6] + m, 58 << 24)
    return MAC + PEER_MAC + b"\x86\xdd" + h + m[:2] + ck + m[4:]


def frame(kind: str, rng) -> bytes:
    if kind == "udp":
        return template("udp", rng)
    if kind == "arp_us":
        return arp(1, A4, rng)
    if kind == "arp_other":
        return arp(1, bytes((10, 1, 0, int(rng.integers(2, 250)))), rng)
    if kind == "arp_reply":
        return arp(2, A4, rng, dst=MAC)
    return nsol(rng)


def build_ring(dev, n: int, ring: str, seed: int):
    rng = np.random.default_rng(seed)
    if ring == "mixed":
        kinds = [("arp_us" if (t // 3) % 8 == 0 else "arp_reply" if (t // 3) % 8 == 4 else "arp_other")
                 if t % 3 == 0 else "udp" for t in range(TEMPLATES)]
    else:
        kinds = ["arp_us" if ring == "arp" else "nsol"] * TEMPLATES
    block = np.zeros((TEMPLATES, SLOT), np.uint8)
    lens = np.empty(TEMPLATES, np.uint16)
    for t, kind in enumerate(kinds):
        fr = frame(kind, rng)
        block[t, :len(fr)], lens[t] = np.frombuffer(fr, np.uint8), len(fr)
    reps = n // TEMPLATES
    buf = torch.from_numpy(block.reshape(-1)).to(dev).repeat(reps)
    buf = torch.cat([buf, torch.zeros(64, dtype=torch.uint8, device=dev)])
    f_off = (np.arange(n, dtype=np.uint64) * SLOT)
    return buf, f_off, np.tile(lens, reps), np.array(kinds * reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", choices=("mixed", "arp", "nsol"), default="mixed")
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wc.gpu_init(0)
    n = args.frames // TEMPLATES * TEMPLATES
    rings = [build_ring(dev, n, args.ring, 11 + 7 * r) for r in range(args.rings)]
    eng = torch.from_numpy(engine().view(np.uint8)).to(dev)
    _, f_off, _, kinds = rings[0]
    d_off = torch.from_numpy(f_off).to(dev)
    d_lens = [torch.from_numpy(r[2]).to(dev) for r in rings]
    want_exp = np.array([CODE[k] for k in kinds], np.uint8)
    n_upd = int(((wc.RN_MASK_UPDATE >> want_exp.astype(np.uint32)) & 1).sum())
    n_rep = int(((wc.RN_MASK_REPLY >> want_exp.astype(np.uint32)) & 1).sum())
    rep_len = 42 if args.ring != "nsol" else 86
    out = torch.empty(max(n_rep, 1) * 128 + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(n_rep, dtype=torch.int64, device=dev) * 128
    state = {}

    def front(r):
        v, _ = wc.rx_verdict_ragged(rings[r][0], d_off, d_lens[r], check=False)
        state[r] = v

    def rplan(r):
        state[r, "act"] = wc.rx_reply_plan(rings[r][0], d_off, d_lens[r], state[r], None, eng, SLOT,
                                           want_list=False, check=False)[0]

    def nplan(r, lists=True):
        res = wc.rx_neigh_plan(rings[r][0], d_off, d_lens[r], state[r, "act"], eng,
                               want_replies=lists, want_updates=lists, check=False)
        if lists:
            state[r, "plan"] = res

    def updates(r):
        nact, _, _, ul, uc = state[r, "plan"]
        state[r, "upd"] = wc.rx_neigh_updates(rings[r][0], d_off, d_lens[r], nact, ul, uc, n_upd,
                                              check=False)

    def build(r):
        nact, rl, rcnt, _, _ = state[r, "plan"]
        state[r, "built"] = wc.rx_neigh_build(rings[r][0], d_off, d_lens[r], nact, rl, rcnt, eng, out,
                                              o_off, 128, check=False)

    print(f"== ring {args.ring}: {n} frames in {SLOT}-B slots, {args.rings} buffers; {n_upd} cache "
          f"updates and {n_rep} replies of {rep_len} bytes per ring", flush=True)
    for r in range(args.rings):
        front(r), rplan(r), nplan(r), updates(r), build(r)
        nact, _, rcnt, _, ucnt = state[r, "plan"]
        a = state[r, "act"].cpu().numpy()
        host = np.where(rings[r][3] == "udp", wc.RR_NONE, wc.RR_HOST)
        u = state[r, "upd"].cpu().numpy().view(wc.NEIGH_UPDATE).reshape(-1)
        olen, built = state[r, "built"]
        ok = bool((a == host).all()) and bool((nact.cpu().numpy() == want_exp).all()) and \
            int(rcnt.item()) == n_rep and int(ucnt.item()) == n_upd and int(built.item()) == n_rep and \
            bool((olen.cpu().numpy() == rep_len).all()) and \
            bool((u["af"] == (6 if args.ring == "nsol" else 4)).all())
        print(f"check, buffer {r}: actions, codes, {n_upd} records and {n_rep} replies equal the "
              f"classes: {ok}", flush=True)
        if not ok:
            raise SystemExit("neighbour check failed")
    names = ("reply_plan", "neigh_plan", "neigh_plan_lists", "updates", "build")
    ts = {k: [] for k in names}
    for i in range(args.warmup + args.rounds):
        r = i % args.rings
        t = {"reply_plan": timed(lambda: rplan(r)), "neigh_plan": timed(lambda: nplan(r, False)),
             "neigh_plan_lists": timed(lambda: nplan(r)), "updates": timed(lambda: updates(r)),
             "build": timed(lambda: build(r))}
        tag = "warm" if i < args.warmup else "round"
        print(f"{tag} {i:2d}: reply plan alone {t['reply_plan'] * 1e6:7.1f} us | neigh plan alone "
              f"{t['neigh_plan'] * 1e6:7.1f} us | with lists {t['neigh_plan_lists'] * 1e6:7.1f} us | "
              f"updates {t['updates'] * 1e6:7.1f} us | build {t['build'] * 1e6:7.1f} us", flush=True)
        if i >= args.warmup:
            for k in ts:
                ts[k].append(t[k])
    print(f"== medians over {args.rounds} rounds (min .. max), us: " + "; ".join(
        f"{k} {statistics.median(v) * 1e6:.1f} ({min(v) * 1e6:.1f} .. {max(v) * 1e6:.1f})"
        for k, v in ts.items()), flush=True)
    mb = statistics.median(ts["build"])
    print(f"== build: {mb / max(n_rep, 1) * 1e9:.2f} ns per reply, updates: "
          f"{statistics.median(ts['updates']) / max(n_upd, 1) * 1e9:.2f} ns per record")
    print("(device-event times of single calls, Python wrappers and their allocations included; "
          "kernel times: rocprofv3 --kernel-trace --stats)")


if __name__ == "__main__":
    main()
