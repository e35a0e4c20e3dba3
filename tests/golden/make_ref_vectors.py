"""Regenerate tests/golden/ref_vectors.npz: results recorded from the
reference's own checksum object (oracle/ref_oracle.py -> oracle/_ref/
libwc_ref.so, lib/src/in_cksum.c of the reference compiled unchanged).

A GPU host has no reference tree, so the GPU tests (tests/test_gpu_parity.py)
run against this file; tests/test_reference.py recomputes every *_expect with
the live object wherever that exists, so the file cannot drift from the
reference unnoticed.  Needs the reference tree (WC_REFERENCE_DIR).

Groups, in the *_blob / *_off / *_len / *_expect layout of vectors.npz:

ip   one random blob; starts 0..15 x lengths 0..130, 255..257, 1471..1473,
     9000, 9001, 65535                                       -> ip_cksum
pl   450 wild + 150 plain UDP packets (payload <= 300 B; both versions, IHL
     5..15, bad total lengths, next_hdr 0..255) and four MTU-size IPv6 packets
     with next_hdr 255 / 254 over random bodies (the uint32 wrap at an
     everyday size), at align 1, lead 7; one 65535-byte IPv6 packet, next_hdr
     255, all-0xFF payload (the wrap again); every version nibble x IHL
     nibble, with and without a body                         -> payload_cksum
fu   the first 604 packets of pl (fu_off / fu_len point into pl_blob)
     -> fu_hdr_expect = ip_cksum(ip, hl) for IPv4, 0 for IPv6, and
        fu_pl_expect = payload_cksum, as wc_cksum_ip_udp_* returns them
st   strided, 256 packets at each (length, stride) of refcases.ST_SHAPES.
     Only the headers are stored (st<k>_hdr): the bodies are the project's
     counter-based byte stream under seed st_seed + k, rebuilt by
     refcases.st_blob -- 0.9 MB of random bodies would not fit a fixture.
     -> st<k>_ip_expect, st<k>_pl_expect, st<k>_hdr_expect (as fu_hdr_expect)
tx   Ethernet frames around the fu packets with both checksum fields
     overwritten (refcases.tx_frames): tests/tx_model.py's seal with its two
     checksum calls answered by the reference
     -> tx_status, tx_hdr_expect, tx_udp_expect (0 where none is computed)

    python tests/golden/make_ref_vectors.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import refcases  # noqa: E402
import tx_model  # noqa: E402
from packets import ipv6_udp, pack, random_packets  # noqa: E402

SEED = 0x4EF0
ST_SEED = 0x57A1D


def inputs() -> dict:
    rng = np.random.default_rng(SEED)
    g = {"ip_blob": rng.integers(0, 256, 65535 + 15 + 64, dtype=np.uint8)}
    g["ip_off"], g["ip_len"] = refcases.ip_sweep(refcases.IP_LENS_FIXTURE)

    udp = random_packets(rng, 450, max_payload=300, wild=True) \
        + random_packets(rng, 150, max_payload=300) \
        + [ipv6_udp(rng.integers(0, 256, p, dtype=np.uint8).tobytes(), rng, next_hdr=nh)
           for p, nh in ((1472, 255), (1471, 255), (1472, 254), (1400, 255))]
    pkts = udp + [ipv6_udp(bytes([0xFF]) * 65487, rng, next_hdr=255)] \
        + refcases.nibble_grid_packets(rng)
    g["pl_blob"], g["pl_off"], g["pl_len"] = pack(pkts, align=1, lead=7)
    g["fu_off"], g["fu_len"] = g["pl_off"][: len(udp)].copy(), g["pl_len"][: len(udp)].copy()

    g["st_seed"] = np.uint64(ST_SEED)
    for k, (length, _) in enumerate(refcases.ST_SHAPES):
        g[f"st{k}_hdr"] = refcases.st_headers(rng, length)
    return g


def main():
    g = inputs()
    g.update(refcases.expects(g))
    out = refcases.REF_VECTORS
    np.savez_compressed(out, **g)
    print(f"{out.name}: {out.stat().st_size} bytes; ip {g['ip_off'].size}, pl {g['pl_off'].size}, "
          f"fu {g['fu_off'].size}, st {len(refcases.ST_SHAPES)} x {refcases.ST_N}, "
          f"tx sealed {int((g['tx_status'] == tx_model.SEALED).sum())}")


if __name__ == "__main__":
    main()
