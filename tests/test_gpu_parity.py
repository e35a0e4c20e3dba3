"""GPU parity tests: the gfx950 kernels (through the C ABI) against the CPU
oracle on the same bytes -- bit-exact, every packet.

Sizes: the golden fixtures and edge sweeps are small; the BASELINE.json
configurations C2 (2^20 x 1472 B), C3 (MTU sweep x 2^20) and C4 (2^24 Zipf
packets, packed unaligned) are checked in full against the multi-threaded C
oracle.
"""
import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import refcases
import tx_model
import warpcore_amd as wc
from oracle import c_oracle, py_oracle
from packets import (insert_checksum, ipv4_udp, ipv6_udp, pack, random_packets, rx_ring,
                     slot_ring)
from test_gpu_tx import assert_same_bytes
from warpcore_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
ROOT = Path(__file__).resolve().parent.parent


def to_dev(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_u8(a: np.ndarray, dev, pad: int = 64) -> torch.Tensor:
    """Device copy with 16-byte aligned base and `pad` spare bytes."""
    t = torch.zeros(a.size + pad, dtype=torch.uint8, device=dev)
    t[: a.size] = torch.from_numpy(np.ascontiguousarray(a))
    return t


def host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint16)


# Ragged kernel paths (wc_cksum_api.cpp plan_ragged, k_cksum_seg): the flat
# kernel alone; the seg kernel without its grouped path; the grouped path
# forced for every tile; and the default per-tile choice.
RAGGED_MODES = {
    "flat": {"WC_SEG": "0"},
    "flat2": {"WC_SEG": "0", "WC_FLAT_PK": "2"},
    "seg": {"WC_SEG": "1", "WC_GRP_DENSE": "65", "WC_GRP_SPARSE": "65"},
    "grp": {"WC_SEG": "1", "WC_GRP_DENSE": "0", "WC_GRP_SPARSE": "0"},
    "segflat": {"WC_SEG": "1", "WC_GATHER": "0"},
    "gath": {"WC_SEG": "1", "WC_GATHER": "2", "WC_GRP_DENSE": "65", "WC_GRP_SPARSE": "65"},
    # the gathered stream's end-bit owner lookup with 2- and 8-row groups
    "gath2": {"WC_SEG": "1", "WC_GATHER": "2", "WC_GRP_DENSE": "65", "WC_GRP_SPARSE": "65",
              "WC_SEG_ROWS": "2"},
    "gath8": {"WC_SEG": "1", "WC_GATHER": "2", "WC_GRP_DENSE": "65", "WC_GRP_SPARSE": "65",
              "WC_SEG_ROWS": "8"},
    "default": {},
}


def ragged_mode(monkeypatch, mode: str) -> None:
    for k in ("WC_SEG", "WC_GRP_DENSE", "WC_GRP_SPARSE", "WC_FLAT_PK", "WC_VARIANT", "WC_GATHER",
              "WC_SEG_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in RAGGED_MODES[mode].items():
        monkeypatch.setenv(k, v)
    wc.reload_config()  # the library reads WC_* once; re-read for this test


# ---------------------------------------------------------------------------
# Known answers and golden vectors.

def test_kat_scalar_dropin(gpu):
    kat = json.loads((GOLDEN / "kat.json").read_text())
    for case in kat["ip_cksum"]:
        if "hex_repeat" in case:
            b, k = case["hex_repeat"]
            data = bytes.fromhex(b) * k
        else:
            data = bytes.fromhex(case["hex"])
        buf = data if data else b"\x00"
        assert wc.ip_cksum(buf, len(data)) == int(case["expect"], 16), case["name"]


def test_golden_vectors_ip(gpu):
    g = np.load(GOLDEN / "vectors.npz")
    out = wc.cksum_ragged(dev_u8(g["ip_blob"], gpu), to_dev(g["ip_off"], gpu),
                          to_dev(g["ip_len"], gpu), kind="ip")
    np.testing.assert_array_equal(host(out), g["ip_expect"])


def test_golden_vectors_payload(gpu):
    g = np.load(GOLDEN / "vectors.npz")
    out = wc.cksum_ragged(dev_u8(g["pl_blob"], gpu), to_dev(g["pl_off"], gpu),
                          to_dev(g["pl_len"], gpu), kind="payload")
    np.testing.assert_array_equal(host(out), g["pl_expect"])


# ---------------------------------------------------------------------------
# Results recorded from the reference's own in_cksum.c (tests/golden/
# ref_vectors.npz, make_ref_vectors.py): every entry point of the library
# against what the reference computed, not against a restatement of it.  The
# file's groups: ip (start phase x length), pl (wild and plain UDP packets,
# the 65535-byte IPv6 next_hdr wrap, every version x IHL nibble), fu (the UDP
# packets of pl: header checksum and payload_cksum), st (strided shapes,
# bodies rebuilt by refcases.st_blob), tx (the seal's two stored values).

@functools.lru_cache(maxsize=None)
def ref_vectors():
    g = dict(np.load(refcases.REF_VECTORS))
    for k in range(len(refcases.ST_SHAPES)):
        g[f"st{k}_blob"] = refcases.st_blob(g, k)
    g["tx_buf"], g["tx_off"], g["tx_len"] = refcases.tx_frames(g)
    return g  # shared by the tests below and never written


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("group,kind", [("ip", "ip"), ("pl", "payload")])
def test_ref_vectors_ragged(gpu, monkeypatch, group, kind, mode):
    ragged_mode(monkeypatch, mode)
    g = ref_vectors()
    out = wc.cksum_ragged(dev_u8(g[group + "_blob"], gpu), to_dev(g[group + "_off"], gpu),
                          to_dev(g[group + "_len"], gpu), kind=kind)
    np.testing.assert_array_equal(host(out), g[group + "_expect"])


@pytest.mark.parametrize("kind", ["ip", "payload"])
@pytest.mark.parametrize("k", range(len(refcases.ST_SHAPES)))
def test_ref_vectors_strided(gpu, k, kind):
    g = ref_vectors()
    length, stride = refcases.ST_SHAPES[k]
    out = wc.cksum_strided(dev_u8(g[f"st{k}_blob"], gpu, pad=0), stride, length, refcases.ST_N,
                           kind=kind)
    np.testing.assert_array_equal(host(out), g[f"st{k}_{'ip' if kind == 'ip' else 'pl'}_expect"])


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
def test_ref_vectors_fused_ragged(gpu, monkeypatch, mode):
    ragged_mode(monkeypatch, mode)
    g = ref_vectors()
    hdr, pay = wc.cksum_ip_udp_ragged(dev_u8(g["pl_blob"], gpu), to_dev(g["fu_off"], gpu),
                                      to_dev(g["fu_len"], gpu))
    np.testing.assert_array_equal(host(hdr), g["fu_hdr_expect"])
    np.testing.assert_array_equal(host(pay), g["fu_pl_expect"])


@pytest.mark.parametrize("k", range(len(refcases.ST_SHAPES)))
def test_ref_vectors_fused_strided(gpu, k):
    g = ref_vectors()
    length, stride = refcases.ST_SHAPES[k]
    hdr, pay = wc.cksum_ip_udp_strided(dev_u8(g[f"st{k}_blob"], gpu, pad=0), stride, length,
                                       refcases.ST_N)
    np.testing.assert_array_equal(host(hdr), g[f"st{k}_hdr_expect"])
    np.testing.assert_array_equal(host(pay), g[f"st{k}_pl_expect"])


@pytest.mark.parametrize("register", [False, True])
@pytest.mark.parametrize("group,kind", [("ip", "ip"), ("pl", "payload")])
def test_ref_vectors_host(gpu, group, kind, register):
    """wc_cksum_host on pageable and registered memory: the whole group (one
    zero-copy launch or the pipeline), then its first 256 packets of at most
    4064 bytes, which a registered buffer hands to the resident server."""
    g = ref_vectors()
    buf = g[group + "_blob"].copy()
    offs, lens, want = g[group + "_off"], g[group + "_len"], g[group + "_expect"]
    few = np.flatnonzero(lens <= 4064)[:256]
    if register:
        wc.host_register(buf)
    try:
        got = wc.cksum_host(buf, offs, lens, kind=kind)
        s0 = wc.server_stats()
        small = wc.cksum_host(buf, offs[few], lens[few], kind=kind)
        s1 = wc.server_stats()
    finally:
        if register:
            wc.host_unregister(buf)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(small, want[few])
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (int(register), 0)


@pytest.mark.parametrize("register", [False, True])
def test_ref_vectors_fused_host(gpu, register):
    g = ref_vectors()
    buf = g["pl_blob"].copy()
    if register:
        wc.host_register(buf)
    try:
        hdr, pay = wc.cksum_ip_udp_host(buf, g["fu_off"], g["fu_len"])
        s0 = wc.server_stats()
        hdr_s, pay_s = wc.cksum_ip_udp_host(buf, g["fu_off"][:256], g["fu_len"][:256])
        s1 = wc.server_stats()
    finally:
        if register:
            wc.host_unregister(buf)
    np.testing.assert_array_equal(hdr, g["fu_hdr_expect"])
    np.testing.assert_array_equal(pay, g["fu_pl_expect"])
    np.testing.assert_array_equal(hdr_s, g["fu_hdr_expect"][:256])
    np.testing.assert_array_equal(pay_s, g["fu_pl_expect"][:256])
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (int(register), 0)


def test_ref_vectors_scalar_dropin(gpu):
    """ip_cksum / payload_cksum under the reference's own names, 64 cases of
    each spread over the groups (the 65535-byte wrap packet among them)."""
    g = ref_vectors()
    blob, offs, lens = g["ip_blob"], g["ip_off"], g["ip_len"]
    for i in np.linspace(0, offs.size - 1, 64).astype(int).tolist():
        o, n = int(offs[i]), int(lens[i])
        assert wc.ip_cksum(blob[o:o + max(n, 1)], n) == g["ip_expect"][i], i
    blob, offs, lens = g["pl_blob"], g["pl_off"], g["pl_len"]
    pick = set(np.linspace(0, offs.size - 1, 63).astype(int).tolist())
    pick.add(int(np.argmax(lens)))
    assert len(pick) == 64
    for i in sorted(pick):
        o, n = int(offs[i]), int(lens[i])
        assert wc.payload_cksum(blob[o:o + max(n, 40)], n) == g["pl_expect"][i], i


def test_ref_vectors_tx_seal(gpu):
    """wc_tx_seal_ragged on Ethernet frames around the fu packets: the status
    codes and both values are the recorded ones (tests/tx_model.py's chain,
    the two checksums by the reference with both fields zeroed), and the two
    fields of every sealed frame hold them, stored raw."""
    g = ref_vectors()
    buf, offs, lens = g["tx_buf"], g["tx_off"], g["tx_len"]
    d = to_dev(buf, gpu)
    status, hdr, udp, _ = wc.tx_seal_ragged(d, to_dev(offs, gpu), to_dev(lens, gpu))
    np.testing.assert_array_equal(status.cpu().numpy(), g["tx_status"])
    np.testing.assert_array_equal(hdr.cpu().numpy().view(np.uint16), g["tx_hdr_expect"])
    np.testing.assert_array_equal(udp.cpu().numpy().view(np.uint16), g["tx_udp_expect"])
    sealed = d.cpu().numpy()

    def field(at):  # a native uint16 at any address
        return int(sealed[at]) | (int(sealed[at + 1]) << 8)

    checked = 0
    for i, o in enumerate(offs.astype(np.int64).tolist()):
        ip = o + 14
        v4 = sealed[ip] >> 4 == 4
        hl = int(sealed[ip] & 0x0F) * 4 if v4 else 40
        if g["tx_status"][i] in (tx_model.SEALED, tx_model.IP_ONLY):
            assert v4 or g["tx_status"][i] == tx_model.SEALED
            if v4:
                assert field(ip + 10) == g["tx_hdr_expect"][i], i
        if g["tx_status"][i] == tx_model.SEALED:
            assert field(ip + hl + 6) == g["tx_udp_expect"][i], i
            checked += 1
    assert checked > 300


def test_live_reference_ragged(gpu):
    """One live pass where the reference's object came with the tree: 2000
    fresh wild packets, the kernels against the object itself.  (The recorded
    results above are the tests that count; this one may skip.)"""
    from oracle import ref_oracle
    if not ref_oracle.available():
        pytest.skip("no oracle/_ref/libwc_ref.so on this host and no reference tree to build it")
    rng = np.random.default_rng(77)
    buf, offs, lens = pack(random_packets(rng, 2000, max_payload=1472, wild=True), 1, 3)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                               kind="payload"))
    np.testing.assert_array_equal(got, ref_oracle.cksum_ragged(buf, offs, lens, kind=1))


# ---------------------------------------------------------------------------
# Edge sweeps: lengths x start alignment x stride, both batch layouts.

SWEEP_LENS = list(range(0, 131)) + [255, 256, 257, 511, 575, 576, 577, 784, 785, 880, 900,
                                    1000, 1008, 1024, 1040, 1100, 1216, 1232, 1250, 1376,
                                    1392, 1471, 1472, 1473, 1536, 2048, 4095, 8999, 9000,
                                    9001, 65535]


@pytest.mark.parametrize("group,kind", [("icmp", 0), ("ip4hdr", 0), ("udp6", 1), ("udp4", 1)])
def test_linux_kernel_vectors(gpu, group, kind):
    """Checksums computed (or accepted) by the Linux kernel's RFC 1071 code on
    the same bytes: ICMP echo replies, IPv4 headers, UDP over IPv6 / IPv4
    (tests/golden/make_kernel_vectors.py) -- an implementation independent of
    this project and of the reference."""
    g = np.load(GOLDEN / "linux_vectors.npz")
    out = wc.cksum_ragged(dev_u8(g[group + "_blob"], gpu), to_dev(g[group + "_off"], gpu),
                          to_dev(g[group + "_len"], gpu), kind=kind)
    np.testing.assert_array_equal(host(out), g[group + "_expect"])


@pytest.mark.parametrize("length", SWEEP_LENS)
def test_strided_sweep(gpu, length):
    rng = np.random.default_rng(length)
    n = 37
    for stride in sorted({max(length, 1), (length + 15) // 16 * 16 or 16, length + 1}):
        buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
        d = dev_u8(buf, gpu)
        for start in (0, 1, 2, 3, 7, 8, 14, 15):
            if start + (n - 1) * stride + length > buf.size:
                continue
            got = host(wc.cksum_strided(d, stride, length, n, kind="ip", byte_offset=start))
            want = c_oracle.cksum_strided(buf, stride, length, n, kind=0, byte_offset=start)
            np.testing.assert_array_equal(got, want, err_msg=f"stride {stride} start {start}")


# The planner's tuned shapes for the configurations the bench quotes
# (wc_cksum_api.cpp shape_for_chunks).  A regression
# here moves the headline, so it is pinned.
PLANNED = [
    # base, stride, len, kind, (group, chunks per lane, packets per group)
    (0, 1472, 1472, "ip", (32, 4, 1)),        # C2
    (0, 1472, 1472, "payload", (16, 6, 2)),   # C2 as payload_cksum
    (14, 2048, 1500, "ip", (32, 4, 1)),       # netmap slots, strided
    (14, 2048, 1500, "payload", (32, 3, 2)),
    (0, 1024, 1024, "ip", (32, 4, 2)),
    (0, 64, 64, "ip", (4, 1, 4)),             # C3 64 B (lean kernel)
    (0, 256, 256, "ip", (8, 2, 2)),           # lean kernel, the pass filled exactly
    (0, 576, 576, "ip", (16, 3, 1)),
    (0, 9000, 9000, "ip", (32, 18, 1)),
    (14, 2048, 64, "ip", (8, 1, 4)),          # small packets in netmap slots: group kernel
    (14, 2048, 128, "ip", (8, 3, 2)),         # (ip_cksum gains nothing on the PH path)
    (14, 2048, 64, "payload", (8, 1, 4)),     # payload_cksum: lean kernel, PH path
    (14, 2048, 128, "payload", (8, 2, 4)),
    (14, 2048, 240, "payload", (8, 2, 4)),
]


@pytest.mark.parametrize("base,stride,length,kind,shape", PLANNED)
def test_planner_shapes(gpu, monkeypatch, base, stride, length, kind, shape):
    for k in ("WC_SHAPE", "WC_STRIDED_SEG", "WC_VARIANT", "WC_LEAN_MAX", "WC_LEAN_PHASE"):
        monkeypatch.delenv(k, raising=False)
    wc.reload_config()
    p = wc.plan_strided(0x100000000 + base, stride, length, 1 << 20, kind=kind)
    assert (p["group"], p["chunks_per_lane"], p["unroll"]) == shape


@pytest.mark.parametrize("length,seg", [(64, False), (80, True), (144, True), (240, True),
                                        (256, False), (288, False)])
def test_planner_aligned_small_take_seg(gpu, monkeypatch, length, seg):
    """Packed aligned 5..16-chunk packets (stride % 64 != 0) take the seg
    kernel (group 0 in the plan), 64 / 256 B and longer ones the group kernel."""
    for k in ("WC_SHAPE", "WC_STRIDED_SEG", "WC_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    wc.reload_config()
    p = wc.plan_strided(0x100000000, length, length, 1 << 20, kind="ip")
    assert (p["group"] == 0) == seg


@pytest.mark.parametrize("length,kernel", [(64, "lean"), (128, "lean"), (256, "lean"),
                                           (576, "seg"), (992, "seg"), (1024, "group"),
                                           (1472, "group")])
def test_planner_payload_packed(gpu, monkeypatch, length, kernel):
    """payload_cksum, packed: aligned packets whose chunk count a lean group
    pass fills exactly take the lean kernel; the rest below 64 chunks the
    seg kernel; longer ones the group kernel."""
    for k in ("WC_SHAPE", "WC_STRIDED_SEG", "WC_VARIANT", "WC_LEAN_MAX"):
        monkeypatch.delenv(k, raising=False)
    wc.reload_config()
    p = wc.plan_strided(0x100000000, length, length, 1 << 20, kind="payload")
    assert p["kernel"] == kernel
    assert (p["group"] == 0) == (kernel == "seg")


def test_capped_grid_overlapping_stride(gpu):
    """More packets than one grid can hold: 2^26 + 1000 overlapping 3000-B
    packets at stride 16 take the (64,4,1) shape (one packet per wave), whose
    one-shot grid would need 2^24 + 250 workgroups -- more than gridDim.x *
    256 threads fits in a uint32 on AMD.  The launcher caps the grid at
    kMaxGridBlocks and the kernel grid-strides over the rest.
    The packets around the wrap, both ends and a random sample are checked
    against the oracle."""
    n, stride, length = (1 << 26) + 1000, 16, 3000
    d = torch.empty((n - 1) * stride + length + 64, dtype=torch.uint8, device=gpu)
    wc.synth_fill(d, 26)
    got = host(wc.cksum_strided(d, stride, length, n, kind="ip"))
    wrap = ((1 << 24) - 1) * 4  # first packet of the second grid-stride pass
    rng = np.random.default_rng(26)
    idx = np.unique(np.concatenate([np.arange(0, 1000), np.arange(wrap - 1000, wrap + 1000),
                                    np.arange(n - 2000, n), rng.integers(0, n, 20000)]))
    buf = d.cpu().numpy()
    want = c_oracle.cksum_ragged(buf, (idx * stride).astype(np.uint64),
                                 np.full(idx.size, length, np.uint16), kind=0)
    np.testing.assert_array_equal(got[idx], want)
    del d, buf


@pytest.mark.parametrize("sseg", ["0", "1", "2"])
@pytest.mark.parametrize("length", [1, 2, 15, 16, 17, 63, 64, 65, 80, 96, 100, 111, 128, 144, 160,
                                    240, 255, 256, 257, 400, 500, 512, 513, 576, 577, 767, 768,
                                    1472, 1500, 9000])
def test_strided_packed_seg(gpu, monkeypatch, length, sseg):
    """Packed strided batches (stride = len .. len + len / 8) through the seg
    kernel with computed offsets (WC_STRIDED_SEG: 0 = group kernel only,
    1 = planner default, 2 = seg kernel whenever packed): several tiles and
    a partial one, every start phase, ip_cksum and payload_cksum."""
    monkeypatch.setenv("WC_STRIDED_SEG", sseg)
    wc.reload_config()
    rng = np.random.default_rng(length * 7 + int(sseg))
    n = 150
    for stride in sorted({length, length + 1, length + length // 8}):
        buf = rng.integers(0, 256, n * stride + 64 + 16, dtype=np.uint8)
        d = dev_u8(buf, gpu)
        for start in (0, 1, 6, 14, 15):
            got = host(wc.cksum_strided(d, stride, length, n, kind="ip", byte_offset=start))
            want = c_oracle.cksum_strided(buf, stride, length, n, kind=0, byte_offset=start)
            np.testing.assert_array_equal(got, want, err_msg=f"ip stride {stride} start {start}")
        if length >= 48:  # payload_cksum: well-formed UDP headers, then the RX check
            hb = buf.copy()
            for i in range(n):
                o = 14 + i * stride
                pl = rng.integers(0, 256, length - 28 - (20 if i % 3 == 0 else 0),
                                  dtype=np.uint8).tobytes()
                pkt, ln = (ipv6_udp if i % 3 == 0 else ipv4_udp)(pl, rng)
                hb[o:o + ln] = np.frombuffer(pkt, np.uint8)
            d = dev_u8(hb, gpu)
            got = host(wc.cksum_strided(d, stride, length, n, kind="payload", byte_offset=14))
            want = c_oracle.cksum_strided(hb, stride, length, n, kind=1, byte_offset=14)
            np.testing.assert_array_equal(got, want, err_msg=f"payload stride {stride}")


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
def test_ragged_random_placement(gpu, monkeypatch, mode):
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    n = 20000
    lens = rng.integers(0, 9001, n).astype(np.uint16)
    lens[:100] = 0
    lens[100:200] = 1
    offs = rng.integers(0, buf.size - 9001, n).astype(np.uint64)  # overlapping, unsorted
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu)))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=0))


def _sorted_layout(rng, n, lens, gap_max=0, overlap_max=0, lead=0):
    """Packets in offset order: each starts `gap` bytes after the previous
    end (gap in [-overlap_max, gap_max]; starts and ends stay non-decreasing)."""
    offs = np.zeros(n, dtype=np.uint64)
    pos, prev_end = lead, lead
    for i in range(n):
        g = int(rng.integers(-overlap_max, gap_max + 1)) if (gap_max or overlap_max) else 0
        start = max(prev_end + g, int(offs[i - 1]) if i else lead)
        offs[i] = start
        prev_end = max(prev_end, start + int(lens[i]))
    return offs, prev_end + 64


DENSE_LAYOUTS = ["packed", "packed_tiny", "gaps", "gaps_wide", "overlap", "exact_groups",
                 "jumbo", "with_empty"]


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("layout", DENSE_LAYOUTS)
def test_ragged_dense_tiles(gpu, monkeypatch, layout, mode):
    """Ordered ragged layouts (the segmented-prefix path for dense tiles, the
    flat path for the rest): packed at every alignment, small gaps, gaps wide
    enough to make some tiles sparse, overlapping ordered packets, tiles
    ending exactly on a row-group boundary, 65535-B packets and empty
    packets -- every packet against the oracle, on every ragged path."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(sum(layout.encode()))
    n = 6000
    lens = rng.integers(1, 2001, n).astype(np.uint16)
    kw = {}
    if layout == "packed_tiny":
        lens = rng.integers(1, 40, n).astype(np.uint16)
    elif layout == "gaps":
        kw = {"gap_max": 60}
    elif layout == "gaps_wide":
        kw = {"gap_max": 700}
    elif layout == "overlap":
        kw = {"overlap_max": 300, "gap_max": 20}
    elif layout == "exact_groups":
        lens[:] = 1024
        n = 64 * 24
        lens = lens[:n]
    elif layout == "jumbo":
        n = 200
        lens = rng.integers(60000, 65536, n).astype(np.uint16)
        lens[::7] = 65535
    elif layout == "with_empty":
        lens[rng.integers(0, n, 40)] = 0
    offs, size = _sorted_layout(rng, n, lens, lead=int(rng.integers(0, 16)), **kw)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    for k in (0, 1):
        if k == 1:
            if layout in ("with_empty", "packed_tiny"):
                continue  # payload_cksum needs len >= header length
            # make every packet a plausible IP header (v4 IHL 5..15 or v6)
            for o, ln in zip(offs.tolist(), lens.tolist()):
                v6 = ln >= 40 and rng.random() < 0.5
                ihl = int(rng.integers(5, min(15, ln // 4) + 1)) if ln >= 20 else 5
                buf[o] = 0x60 if v6 else 0x40 | ihl
            ok = np.array([(buf[o] >> 4 == 6 and ln >= 40) or (buf[o] >> 4 == 4 and ln >= 4 * (buf[o] & 15))
                           for o, ln in zip(offs.tolist(), lens.tolist())])
            sel = np.flatnonzero(ok)
            o_k, l_k = offs[sel], lens[sel]
        else:
            o_k, l_k = offs, lens
        got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(o_k, gpu), to_dev(l_k, gpu),
                                   kind=k))
        np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, o_k, l_k, kind=k),
                                      err_msg=f"{layout} kind {k}")


@pytest.mark.parametrize("shape", ["64,2,1", "64,4,1", "32,2,1", "16,2,2"])
def test_ragged_group_kernel(gpu, monkeypatch, shape):
    """The small-batch ragged group kernel (forced for every batch size):
    golden vectors of both kinds, random overlapping placements with jumbo
    and empty packets, and wild IPv4/IPv6 packets at odd alignment."""
    monkeypatch.setenv("WC_FLAT_MIN", str(1 << 40))
    monkeypatch.setenv("WC_RAGGED_SHAPE", shape)
    wc.reload_config()
    g = np.load(GOLDEN / "vectors.npz")
    for k, pre in ((0, "ip"), (1, "pl")):
        out = wc.cksum_ragged(dev_u8(g[pre + "_blob"], gpu), to_dev(g[pre + "_off"], gpu),
                              to_dev(g[pre + "_len"], gpu), kind=k)
        np.testing.assert_array_equal(host(out), g[pre + "_expect"])
    rng = np.random.default_rng(21)
    buf = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    lens = rng.integers(0, 9001, 5000).astype(np.uint16)
    lens[:50] = 0
    offs = rng.integers(0, buf.size - 9001, lens.size).astype(np.uint64)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu)))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=0))
    pkts = random_packets(rng, 2000, max_payload=1472, wild=True)
    buf, offs, lens = pack(pkts, align=1, lead=5)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                               kind="payload"))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=1))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("kind", ["ip", "payload"])
@pytest.mark.parametrize("shape", ["slots", "slots_jitter", "uniform_packed", "jumbo", "tail"])
def test_ragged_uniform_tiles(gpu, monkeypatch, kind, shape, mode):
    """Uniform-length ragged batches (the grouped path's tiles): a netmap RX
    ring drained into one batch -- 2048-B slots, IP packet at +14
    (backend_netmap.c:379-391, eth.h:44-48) with exact and jittered lengths,
    v4 / v6 mixed -- packed equal packets at odd alignment, 9000-B jumbo
    frames, and a batch whose last tile is partial.  Every packet against
    the oracle."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(sum(shape.encode()) + (kind == "payload"))
    n, slot, at = 3000, 2048, 14
    if shape == "slots":
        lens = np.full(n, 1500, np.int64)
    elif shape == "slots_jitter":
        lens = rng.integers(1300, 1501, n)
    elif shape == "uniform_packed":
        lens = np.full(n, 1001, np.int64)
    elif shape == "jumbo":
        n, slot = 400, 9216
        lens = rng.integers(8900, 9001, n)
    else:  # tail: 64 k + 5 packets
        n = 64 * 7 + 5
        lens = rng.integers(1400, 1501, n)
    if shape == "uniform_packed":
        offs = 3 + np.arange(n, dtype=np.uint64) * 1001
        size = int(offs[-1]) + 1001 + 64
    else:
        offs = np.arange(n, dtype=np.uint64) * slot + at
        size = n * slot + 64
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    if kind == "payload":
        for i, (o, ln) in enumerate(zip(offs.tolist(), lens.tolist())):
            payload = rng.integers(0, 256, ln - 28 - (20 if i % 3 == 0 else 0),
                                   dtype=np.uint8).tobytes()
            pkt, plen = (ipv6_udp if i % 3 == 0 else ipv4_udp)(payload, rng)
            assert plen == ln == len(pkt)
            buf[o:o + ln] = np.frombuffer(pkt, np.uint8)
    lens = lens.astype(np.uint16)
    k = 1 if kind == "payload" else 0
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu), kind=k))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=k))
    if kind == "payload":  # RX verify of the same ring after the TX pass stored them
        for i, (o, ln) in enumerate(zip(offs.tolist(), lens.tolist())):
            pkt = insert_checksum(bytes(buf[o:o + ln]), int(got[i]))
            buf[o:o + ln] = np.frombuffer(pkt, np.uint8)
        v = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu), kind=1))
        assert (v == 0).all()


def test_all_zero_and_all_ones(gpu):
    for fill, want in ((0x00, 0xFFFF), (0xFF, 0x0000)):
        buf = np.full(1472 * 64, fill, dtype=np.uint8)
        got = host(wc.cksum_strided(dev_u8(buf, gpu), 1472, 1472, 64))
        assert (got == want).all()


def test_empty_batch_is_noop(gpu):
    out = torch.full((4,), 7, dtype=torch.int16, device=gpu)
    wc.cksum_strided(torch.zeros(16, dtype=torch.uint8, device=gpu), 16, 16, 0, out=out)
    assert (out.cpu() == 7).all()


# ---------------------------------------------------------------------------
# payload_cksum (pseudo-header) batches.

@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("align,lead", [(1, 0), (1, 3), (2, 14), (16, 14), (16, 0), (4, 1)])
def test_payload_ragged_wild(gpu, monkeypatch, align, lead, mode):
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(100 + align * 17 + lead)
    pkts = random_packets(rng, 3000, max_payload=1472, wild=True)
    buf, offs, lens = pack(pkts, align=align, lead=lead)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                               kind="payload"))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=1))


def test_payload_strided_netmap_layout(gpu):
    """netmap-like slots: 2048-B buffers, IP header at base + 14 (eth.h:44-48)."""
    rng = np.random.default_rng(7)
    n, slot = 4096, 2048
    buf = np.zeros(n * slot + 64, dtype=np.uint8)
    for v6 in (False, True):
        for i in range(n):
            payload = rng.integers(0, 256, 1472 - (20 if v6 else 0), dtype=np.uint8).tobytes()
            pkt, ln = (ipv6_udp if v6 else ipv4_udp)(payload, rng)
            assert ln == 1500
            buf[i * slot + 14: i * slot + 14 + len(pkt)] = np.frombuffer(pkt, np.uint8)
        got = host(wc.cksum_strided(dev_u8(buf, gpu), slot, 1500, n, kind="payload",
                                    byte_offset=14))
        want = c_oracle.cksum_strided(buf, slot, 1500, n, kind=1, byte_offset=14)
        np.testing.assert_array_equal(got, want)


PHASE_LENS = [1, 2, 15, 20, 47, 48, 49, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256,
              300, 511, 600, 700, 750]


@pytest.mark.parametrize("lean_phase", ["1", "0"])
@pytest.mark.parametrize("length", PHASE_LENS)
def test_lean_phase_slots(gpu, monkeypatch, length, lean_phase):
    """Sparse packets at an even start phase (netmap slots, IP header at +14)
    on the lean kernel's PH path (per-slot byte masks, header words by DPP)
    and, with WC_LEAN_PHASE=0, on the group kernel: both kinds, phases 2 / 6 /
    14, a tail wave, and payload headers of every shape -- IPv4 with IHL 5,
    options (IHL 15), malformed IHL 1, IPv6 with next header 254 / 255."""
    monkeypatch.setenv("WC_LEAN_PHASE", lean_phase)
    wc.reload_config()
    rng = np.random.default_rng(length * 7 + int(lean_phase))
    n, stride = 333, 2048
    buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
    for start in (2, 6, 14):
        b = buf.copy()
        for i in range(n):
            o = start + i * stride
            k = i % 5
            if k == 0 and length >= 60:
                b[o] = 0x4F
            elif k == 1:
                b[o] = 0x41
            elif k == 2 and length >= 40:
                b[o] = 0x60
                b[o + 6] = 254 + (i & 1)
            elif k == 3 or (k == 2 and length < 40):
                b[o] = 0x45
            elif ((b[o] & 15) * 4 if (b[o] >> 4) == 4 else 40) > length:
                # a random header longer than the packet (any version but 4
                # is IPv6's 40 bytes): payload_cksum of len < hl reads ~4 GiB
                # in the reference (undefined there)
                b[o] = 0x45
        d = dev_u8(b, gpu)
        for kind, kn in (("ip", 0), ("payload", 1)):
            if kind == "payload" and length < 20:
                continue
            got = host(wc.cksum_strided(d, stride, length, n, kind=kind, byte_offset=start))
            want = c_oracle.cksum_strided(b, stride, length, n, kind=kn, byte_offset=start)
            np.testing.assert_array_equal(got, want, err_msg=f"{kind} start {start}")
    # the phase path is planned for payload_cksum of 48 B up to 18 window
    # chunks at phase 14 (where it measured faster than the group kernel)
    for kind in ("ip", "payload"):
        plan = wc.plan_strided(0x100000000 + 14, stride, length, n, kind=kind)
        want = (lean_phase == "1" and kind == "payload" and length >= 48
                and (14 + length + 15) // 16 <= 18)
        assert (plan["kernel"] == "lean") == want, (kind, plan)


def test_split_bytes_strided(gpu, monkeypatch):
    """WC_SPLIT_BYTES (the default splitter of strided batches, 3 GiB of
    stride per launch) at small sizes: pieces of 64 KiB of stride."""
    monkeypatch.setenv("WC_SPLIT_BYTES", str(1 << 16))
    wc.reload_config()
    try:
        rng = np.random.default_rng(3)
        n = 20000
        for L, stride, at, kind in ((1472, 1472, 0, "ip"), (100, 2048, 14, "payload"),
                                    (64, 64, 0, "ip"), (333, 333, 5, "payload")):
            buf = rng.integers(0, 256, at + n * stride + 64, dtype=np.uint8)
            got = host(wc.cksum_strided(dev_u8(buf, gpu), stride, L, n, kind=kind,
                                        byte_offset=at))
            want = c_oracle.cksum_strided(buf, stride, L, n, kind=0 if kind == "ip" else 1,
                                          byte_offset=at)
            np.testing.assert_array_equal(got, want, err_msg=f"{L} {stride} +{at} {kind}")
    finally:
        monkeypatch.delenv("WC_SPLIT_BYTES")
        wc.reload_config()


@pytest.mark.parametrize("piece", [1, 777, 4096])
def test_split_launches(gpu, monkeypatch, piece):
    """WC_SPLIT_PKTS: a batch larger than the piece runs as back-to-back
    launches of `piece` packets (each piece planned on its own: its base, its
    phase) -- strided (C2-shaped, netmap slots at +14, packed at odd offsets),
    ragged (Zipf, packed), fused, and the verify count, all equal to the
    oracle / to one launch."""
    monkeypatch.setenv("WC_SPLIT_PKTS", str(piece))
    wc.reload_config()
    try:
        rng = np.random.default_rng(piece)
        n = 10000
        for L, stride, at, kind in ((1472, 1472, 0, "ip"), (300, 2048, 14, "payload"),
                                    (200, 201, 3, "ip"), (1500, 1500, 7, "payload")):
            buf = rng.integers(0, 256, at + n * stride + 64, dtype=np.uint8)
            got = host(wc.cksum_strided(dev_u8(buf, gpu), stride, L, n, kind=kind,
                                        byte_offset=at))
            want = c_oracle.cksum_strided(buf, stride, L, n, kind=0 if kind == "ip" else 1,
                                          byte_offset=at)
            np.testing.assert_array_equal(got, want, err_msg=f"{L} {stride} +{at} {kind}")
        lens = synth.zipf_lengths(n, seed=piece)
        offs = synth.packed_offsets(lens, lead=5)
        buf = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 64, dtype=np.uint8)
        d = dev_u8(buf, gpu)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(gpu)
        d_len = torch.from_numpy(lens.astype(np.int16)).to(gpu)
        for kind, k in (("ip", 0), ("payload", 1)):
            got = host(wc.cksum_ragged(d, d_off, d_len, kind=kind))
            np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=k))
        synth.stamp_udp_headers(d, d_off, d_len)
        buf = d.cpu().numpy()[: buf.size]
        hdr, pay = wc.cksum_ip_udp_ragged(d, d_off, d_len)
        want_h, want_p = fused_want(buf, offs, lens)
        np.testing.assert_array_equal(host(hdr), want_h)
        np.testing.assert_array_equal(host(pay), want_p)
        out, bad = wc.verify_ragged(d, d_off, d_len, kind="payload")
        assert int(bad.item()) == int((want_p != 0).sum())
    finally:
        monkeypatch.delenv("WC_SPLIT_PKTS")
        wc.reload_config()


@pytest.mark.parametrize("length", [60, 64, 100, 333, 1000, 1500])
def test_strided_packed_seg_wild_payload(gpu, monkeypatch, length):
    """payload_cksum on the seg-only packed strided kernel with random header
    bytes: IPv4 options up to IHL 15, malformed IHL < 5,
    IPv6 next_hdr 254 / 255 at odd starts (the uint32 wrap the seg arithmetic
    can't follow) -- those lanes are recomputed by their own lane
    (lane_payload_exact), the rest of the tile keeps the seg result."""
    monkeypatch.setenv("WC_STRIDED_SEG", "2")
    wc.reload_config()
    rng = np.random.default_rng(length * 31)
    n = 700
    for stride in sorted({length, length + 1}):
        buf = rng.integers(0, 256, n * stride + 128, dtype=np.uint8)
        for start in (0, 1, 3):
            for i in range(n):
                o = start + i * stride
                kind = i % 5
                if kind == 0:              # IPv4 with options: a 60-B header
                    # (lengths >= 60: a header longer than the packet makes
                    # the reference read ~4 GiB -- undefined, the oracle
                    # faults like it)
                    buf[o] = 0x4F
                elif kind == 1:
                    buf[o] = 0x41          # IPv4, malformed IHL 1
                elif kind == 2:
                    buf[o] = 0x60          # IPv6, next header near 255
                    buf[o + 6] = 254 + (i & 1)
                elif kind == 3:
                    buf[o] = 0x45
            d = dev_u8(buf, gpu)
            got = host(wc.cksum_strided(d, stride, length, n - 1, kind="payload",
                                        byte_offset=start))
            want = c_oracle.cksum_strided(buf, stride, length, n - 1, kind=1, byte_offset=start)
            np.testing.assert_array_equal(got, want, err_msg=f"stride {stride} start {start}")


@pytest.mark.parametrize("length,stride,start", [(1472, 1472, 0), (1500, 2048, 14),
                                                  (1472, 2048, 1), (1536, 2048, 0)])
def test_payload_strided_mtu_header_terms(gpu, length, stride, start):
    """payload_cksum on the 96-chunk group shapes (32 x 3, 16 x 6), which sum
    [8, len) with ip_cksum's masks and add the header terms at the end: a
    round holding an IPv4 header with options, a malformed IHL or a short
    packet is summed again with header ranges.  Every header kind in every
    round position, IPv6 next_hdr 254 / 255 (the uint32 wrap), both parities
    of the start, against the oracle."""
    rng = np.random.default_rng(length + stride + start)
    n = 1500
    buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
    for i in range(n):
        o = start + i * stride
        k = (i * 7) % 11
        if k < 5:
            pkt, ln = (ipv6_udp if k % 2 else ipv4_udp)(
                rng.integers(0, 256, length - 28 - (20 if k % 2 else 0),
                             dtype=np.uint8).tobytes(), rng)
            buf[o:o + ln] = np.frombuffer(pkt, np.uint8)
        elif k == 5:
            buf[o] = 0x40 | int(rng.integers(6, 16))   # IPv4 with options
        elif k == 6:
            buf[o] = 0x40 | int(rng.integers(0, 5))    # malformed IHL < 5
        elif k == 7:
            buf[o] = 0x60                              # IPv6, next_hdr 254 / 255
            buf[o + 6] = 254 + (i & 1)
        # k 8..10: random bytes as they are
    d = dev_u8(buf, gpu)
    got = host(wc.cksum_strided(d, stride, length, n, kind="payload", byte_offset=start))
    want = c_oracle.cksum_strided(buf, stride, length, n, kind=1, byte_offset=start)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("length,stride", [(700, 2048), (1000, 1003), (1500, 1500),
                                           (1500, 2048), (3000, 3001), (3000, 4096),
                                           (5000, 5007)])
def test_payload_strided_group_shapes(gpu, length, stride):
    """payload_cksum on the group kernel's 16-, 32- and 64-lane shapes, whose
    header bytes come by DPP broadcast: random header bytes (every version /
    IHL / length / next-header combination) and well-formed UDP packets, at
    every start phase (a stride that is not a multiple of 16 moves it packet
    by packet)."""
    rng = np.random.default_rng(length + stride)
    n = 600
    buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
    for i in range(0, n, 3):  # every third packet well-formed
        o = 5 + i * stride
        pkt, ln = (ipv6_udp if i % 2 else ipv4_udp)(
            rng.integers(0, 256, length - 28 - (20 if i % 2 else 0), dtype=np.uint8).tobytes(), rng)
        buf[o:o + ln] = np.frombuffer(pkt, np.uint8)
    d = dev_u8(buf, gpu)
    for start in (5, 14):
        got = host(wc.cksum_strided(d, stride, length, n - 1, kind="payload", byte_offset=start))
        want = c_oracle.cksum_strided(buf, stride, length, n - 1, kind=1, byte_offset=start)
        np.testing.assert_array_equal(got, want, err_msg=f"start {start}")


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("align,lead", [(1, 5), (2, 0)])
def test_payload_ipv6_wrap(gpu, monkeypatch, align, lead, mode):
    """The reference's uint32 wrap of next_hdr << 24 (in_cksum.c:157) on
    jumbo IPv6 packets: odd starts (the seg kernel hands such tiles to the
    exact flat path) and even starts (the seg kernel's own exact path)."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(8)
    pkts = [ipv6_udp(bytes([0xFF]) * p, rng, next_hdr=nh)
            for p in (60000, 65000, 65487) for nh in (17, 58, 128, 200, 255)]
    pkts += [ipv6_udp(rng.integers(0, 256, p, dtype=np.uint8).tobytes(), rng, next_hdr=nh)
             for p in (200, 1472, 9000) for nh in (17, 250, 253, 255)]
    # all-0xFF bodies around the length where next_hdr 254 / 255 starts to
    # wrap the uint32 (the seg kernel's seg_wrap_risk bound)
    pkts += [ipv6_udp(bytes([0xFF]) * p, rng, next_hdr=nh)
             for p in range(380, 620, 7) for nh in (254, 255)]
    buf, offs, lens = pack(pkts, align=align, lead=lead)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                               kind="payload"))
    b = buf.tobytes()
    want = [py_oracle.payload_cksum(b[o:o + n], n) for o, n in zip(offs, lens)]
    np.testing.assert_array_equal(got, np.array(want, np.uint16))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("align", [1, 2])
def test_payload_malformed_headers(gpu, monkeypatch, align, mode):
    """Random bytes as IP packets, packed: every version nibble, IHL 0..15
    (IHL < 5 double-counts src/dst like the reference), len == hl (no
    body), next_hdr up to 255 -- every packet against the
    oracle, in dense tiles (seg kernel) and sparse ones."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(31 + align)
    n = 4000
    lens = rng.integers(0, 120, n).astype(np.uint16)
    big = rng.random(n) < 0.3
    lens[big] = rng.integers(1000, 1501, int(big.sum()))
    pkts = []
    for ln in lens.tolist():
        b = bytearray(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
        if rng.random() < 0.4:
            b[0] = 0x40 | int(rng.integers(0, 16))
        elif rng.random() < 0.5:
            b[0] = 0x60 | int(rng.integers(0, 16))
        hl = (b[0] & 15) * 4 if b[0] >> 4 == 4 else 40
        ln = max(ln, hl)  # len < hl: the reference reads ~4 GiB (undefined)
        body = rng.integers(0, 256, max(ln, 40) - 40, dtype=np.uint8).tobytes()
        pkts.append((bytes(b) + body, ln))  # >= 40 bytes: the fields payload_cksum reads
    buf, offs, lens = pack(pkts, align=align, lead=3)
    got = host(wc.cksum_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                               kind="payload"))
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(buf, offs, lens, kind=1))


def test_verify_counts_bad_packets(gpu):
    """RX verification (udp.c:132-139): packets carrying their checksum give 0."""
    rng = np.random.default_rng(9)
    pkts = random_packets(rng, 2000, max_payload=1400)
    fixed, corrupt = [], 0
    for k, (pkt, ln) in enumerate(pkts):
        c = py_oracle.payload_cksum(pkt, ln)
        if c == 0:       # the reference would send 0 = "no checksum" (udp.c:209-213)
            continue
        bad_one = k % 3 == 0
        corrupt += bad_one
        fixed.append((insert_checksum(pkt, c ^ 0x0101 if bad_one else c), ln))
    buf, offs, lens = pack(fixed, align=2, lead=14)
    out, bad = wc.verify_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu),
                                kind="payload")
    res = host(out)
    assert int(bad.item()) == corrupt == int((res != 0).sum())
    np.testing.assert_array_equal(res, c_oracle.cksum_ragged(buf, offs, lens, kind=1))


def test_scalar_payload_dropin(gpu):
    rng = np.random.default_rng(10)
    for pkt, ln in random_packets(rng, 50, max_payload=1472, wild=True):
        assert wc.payload_cksum(pkt, ln) == py_oracle.payload_cksum(pkt, ln)


# ---------------------------------------------------------------------------
# BASELINE.json configurations at full size (bit-exact over all packets).

def synth_batch(gpu, nbytes, seed=synth.SEED):
    d = torch.empty(nbytes + 64, dtype=torch.uint8, device=gpu)
    wc.synth_fill(d, seed, nbytes=nbytes)
    return d


def test_c2_full_1m_x_1472(gpu):
    n, L = 1 << 20, 1472
    d = synth_batch(gpu, n * L)
    got = host(wc.cksum_strided(d, L, L, n))
    hb = d[: n * L].cpu().numpy()
    np.testing.assert_array_equal(hb, c_oracle.synth(n * L, synth.SEED))
    np.testing.assert_array_equal(got, c_oracle.cksum_strided(hb, L, L, n, kind=0))


@pytest.mark.parametrize("L", [64, 256, 576, 1472, 9000])
def test_c3_mtu_sweep_full(gpu, L):
    n = 1 << 20
    d = synth_batch(gpu, n * L, seed=synth.SEED ^ L)
    got = host(wc.cksum_strided(d, L, L, n))
    hb = d[: n * L].cpu().numpy()
    np.testing.assert_array_equal(got, c_oracle.cksum_strided(hb, L, L, n, kind=0))


@pytest.mark.parametrize("mode", ["default", "flat", "flat2"])
def test_c4_zipf_full(gpu, monkeypatch, mode):
    """C4 in full through the seg kernel (default) and the flat kernel."""
    ragged_mode(monkeypatch, mode)
    lens = synth.zipf_lengths(1 << 24)
    offs = synth.packed_offsets(lens)
    total = int(offs[-1]) + int(lens[-1])
    d = synth_batch(gpu, total, seed=synth.ZIPF_SEED)
    got = host(wc.cksum_ragged(d, to_dev(offs, gpu), to_dev(lens, gpu)))
    hb = d[:total].cpu().numpy()
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(hb, offs, lens, kind=0))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("kind,headers", [("ip", False), ("payload", True), ("payload", False)])
def test_zslots_netmap_ring_mixed_sizes(gpu, monkeypatch, kind, headers, mode):
    """A netmap RX ring of mixed sizes (backend_netmap.c:379-391): C4's Zipf
    64-1472 B lengths, one packet per 2048-B slot at +14 (eth.h:44-48) --
    tools/tune.py --config zslots at 2^18 packets -- with well-formed UDP
    headers or random bytes read as IP headers; every packet vs the oracle."""
    ragged_mode(monkeypatch, mode)
    n = 1 << 18
    lens = synth.zipf_lengths(n)
    offs = (np.arange(n, dtype=np.uint64) * 2048 + 14).astype(np.uint64)
    d = synth_batch(gpu, n * 2048, seed=synth.ZIPF_SEED ^ 14)
    d_off, d_len = to_dev(offs, gpu), to_dev(lens, gpu)
    if headers:
        synth.stamp_udp_headers(d, d_off, d_len)
    k = 0 if kind == "ip" else 1
    got = host(wc.cksum_ragged(d, d_off, d_len, kind=kind))
    hb = d[: n * 2048].cpu().numpy()
    np.testing.assert_array_equal(got, c_oracle.cksum_ragged(hb, offs, lens, kind=k))
    if kind == "payload":
        hdr, pay = wc.cksum_ip_udp_ragged(d, d_off, d_len)
        np.testing.assert_array_equal(host(pay), c_oracle.cksum_ragged(hb, offs, lens, kind=1))
        np.testing.assert_array_equal(host(hdr), _ip_hdr_expect_np(hb, offs))


def _ip_hdr_expect_np(buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
    """Vectorised py_oracle.ip_hdr_cksum: ip_cksum(ip, ip4_hl) for IPv4
    (ip4.c:110-115), 0 for IPv6; hl is a multiple of 4, so whole LE words."""
    idx = offs.astype(np.int64)[:, None] + np.arange(60, dtype=np.int64)[None, :]
    b = buf[idx].astype(np.uint32)
    hl = (b[:, 0] & 15) * 4
    words = b[:, 0::2] + (b[:, 1::2] << 8)
    acc = (words * (np.arange(30)[None, :] * 2 < hl[:, None])).sum(axis=1).astype(np.uint64)
    while (acc > 0xFFFF).any():
        acc = (acc & 0xFFFF) + (acc >> 16)
    res = (~acc & 0xFFFF).astype(np.uint16)
    return np.where(b[:, 0] >> 4 == 4, res, 0).astype(np.uint16)


def test_c2_roundtrip_property(gpu):
    """Size-independent check: store each packet's checksum into its first
    two bytes' place (zeroed), re-checksum -> every packet verifies to 0."""
    n, L = 1 << 20, 1472
    d = synth_batch(gpu, n * L, seed=42)
    pk = d[: n * L].view(n, L)
    pk[:, 0:2] = 0
    c = wc.cksum_strided(d, L, L, n)
    pk[:, 0:2] = c.view(torch.int16).view(torch.uint8).view(n, 2)
    out, bad = wc.verify_strided(d, L, L, n, kind="ip")
    assert int(bad.item()) == 0
    assert (out.view(torch.int16) == 0).all()


# ---------------------------------------------------------------------------
# Host-memory (end-to-end) path and the C drop-in.

@pytest.mark.parametrize("kind", ["ip", "payload"])
@pytest.mark.parametrize("register", [False, True])
def test_host_path(gpu, register, kind):
    """Pipelined host path, > 1 chunk, both kinds (payload_cksum: random
    bytes read as IPv4/IPv6 headers, every len >= 64 >= hl; max(len, 20)
    spans and rebased offsets through the seg kernel on the staged bytes)."""
    rng = np.random.default_rng(12)
    lens = synth.zipf_lengths(300000, seed=5)
    offs = synth.packed_offsets(lens, lead=3)
    buf = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 64, dtype=np.uint8)
    if register:
        wc.host_register(buf)
    try:
        got = wc.cksum_host(buf, offs, lens, kind=kind)
    finally:
        if register:
            wc.host_unregister(buf)
    np.testing.assert_array_equal(
        got, c_oracle.cksum_ragged(buf, offs, lens, kind=0 if kind == "ip" else 1))


@pytest.mark.parametrize("kind", ["ip", "payload"])
@pytest.mark.parametrize("n", [1, 64, 4096])
def test_host_zero_copy_small_batches(gpu, kind, n):
    """Registered pool, small batch, slots in pool order scrambled -- the
    socket RX shape (backend_sock.c:145 pool, w_rx batches of 64)."""
    rng = np.random.default_rng(n * 7 + len(kind))
    slot = 2048
    pool = np.zeros(4096 * slot, dtype=np.uint8)
    pool[:] = rng.integers(0, 256, pool.size, dtype=np.uint8)
    if kind == "payload":
        pkts = random_packets(rng, n, max_payload=slot - 80, wild=True)
        lens = np.array([ln for _, ln in pkts], dtype=np.uint16)
    else:
        lens = rng.integers(0, slot - 15, n).astype(np.uint16)
        pkts = None
    slots = rng.permutation(4096)[:n]
    offs = (slots * slot + rng.integers(0, 16, n)).astype(np.uint64)
    if pkts is not None:
        for o, (p, _) in zip(offs, pkts):
            pool[int(o): int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    want = c_oracle.cksum_ragged(pool, offs, lens, kind=0 if kind == "ip" else 1)
    wc.host_register(pool)
    try:
        got = wc.cksum_host(pool, offs, lens, kind=kind)
    finally:
        wc.host_unregister(pool)
    np.testing.assert_array_equal(got, want)


def fused_want(pool, offs, lens):
    """The fused TX pair by the oracle: ip_cksum(pkt, hl) of each IPv4 packet
    (0 for IPv6) and payload_cksum(pkt, len) (ip4.c:184-186, udp.c:209-213)."""
    b0 = pool[offs.astype(np.int64)]
    v4 = (b0 >> 4) == 4
    hl = np.where(v4, (b0 & 0x0F).astype(np.uint16) * 4, 0).astype(np.uint16)
    hdr = np.where(v4, c_oracle.cksum_ragged(pool, offs, hl, kind=0), 0).astype(np.uint16)
    return hdr, c_oracle.cksum_ragged(pool, offs, lens, kind=1)


@pytest.mark.parametrize("n,register", [(1, True), (64, True), (256, True), (1000, True),
                                        (6000, True), (64, False), (3000, False)])
def test_host_fused_ip_udp(gpu, n, register):
    """wc_cksum_ip_udp_host: the IPv4 header checksum and payload_cksum of
    host-memory packets in one call -- the resident server (registered, <=
    256 packets), one zero-copy launch (registered, <= 4096), the pipeline
    (larger, or pageable), slots in scrambled order.  Wild headers: IPv4
    options (IHL up to 15), IHL < 5, bad total lengths, IPv6 with any next
    header.  (len >= hl always: payload_cksum of len < hl reads ~4 GiB in
    the reference, in_cksum.c:164.)"""
    rng = np.random.default_rng(n * 3 + register)
    slot = 2048
    nslots = max(n, 64)
    pool = rng.integers(0, 256, nslots * slot + 64, dtype=np.uint8)
    pkts = random_packets(rng, n, max_payload=slot - 100, wild=True)
    slots = rng.permutation(nslots)[:n]
    offs = (slots * slot + rng.integers(0, 16, n)).astype(np.uint64)
    lens = np.array([ln for _, ln in pkts], dtype=np.uint16)
    for o, (p, _) in zip(offs, pkts):
        pool[int(o): int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    want_h, want_p = fused_want(pool, offs, lens)
    if register:
        wc.host_register(pool)
    s0 = wc.server_stats()
    try:
        got_h, got_p = wc.cksum_ip_udp_host(pool, offs, lens)
    finally:
        if register:
            wc.host_unregister(pool)
    s1 = wc.server_stats()
    np.testing.assert_array_equal(got_h, want_h)
    np.testing.assert_array_equal(got_p, want_p)
    served = 1 if register and n <= 256 else 0
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (served, 0)


def test_host_fused_round_trip(gpu):
    """TX -> RX through the host path: both results of wc_cksum_ip_udp_host
    stored raw into headers whose fields were 0 (mk_ip4_hdr, udp_tx), then
    ip_cksum over the header and payload_cksum over the packet give 0 (the RX
    checks, ip4.c:110-115 and udp.c:134) -- and the RX verdict of every frame
    is WC_RX_OK."""
    rng = np.random.default_rng(99)
    n, slot = 200, 2048
    frames = []
    for i in range(n):
        payload = rng.integers(0, 256, int(rng.integers(0, 1400)), dtype=np.uint8).tobytes()
        pkt, ln = (ipv6_udp(payload, rng) if i % 3 == 0 else
                   ipv4_udp(payload, rng, ihl=5 if i % 5 else 7))
        frames.append((pkt, ln))
    pool = np.zeros(n * slot, dtype=np.uint8)
    offs = (np.arange(n) * slot + 14).astype(np.uint64)  # IP header at +14 in a slot
    lens = np.array([ln for _, ln in frames], dtype=np.uint16)
    for o, (p, _) in zip(offs, frames):
        pool[int(o) - 2: int(o)] = [0x86, 0xDD] if p[0] >> 4 == 6 else [0x08, 0x00]
        pool[int(o): int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    wc.host_register(pool)
    try:
        hdr, pay = wc.cksum_ip_udp_host(pool, offs, lens)
        for i, o in enumerate(offs.astype(np.int64)):
            v4 = pool[o] >> 4 == 4
            hl = (pool[o] & 0x0F) * 4 if v4 else 40
            if v4:
                pool[o + 10: o + 12] = np.frombuffer(np.uint16(hdr[i]).tobytes(), np.uint8)
            pool[o + hl + 6: o + hl + 8] = np.frombuffer(np.uint16(pay[i]).tobytes(), np.uint8)
        v4 = (pool[offs.astype(np.int64)] >> 4) == 4
        hl = np.where(v4, (pool[offs.astype(np.int64)] & 0x0F).astype(np.uint16) * 4, 0)
        assert (wc.cksum_host(pool, offs[v4], hl[v4].astype(np.uint16), kind="ip") == 0).all()
        assert (wc.cksum_host(pool, offs, lens, kind="payload") == 0).all()
        verdict, drops = wc.rx_verdict_host(pool, offs - 14, lens + 14)
    finally:
        wc.host_unregister(pool)
    assert drops == 0
    ok = (verdict == wc.RX_OK) | ((verdict == wc.RX_OK_NO_CKSUM) & (pay == 0))
    assert ok.all(), verdict


@pytest.mark.parametrize("waves", ["64", "7"])
def test_host_resident_server(gpu, monkeypatch, waves):
    """Small registered batches answered by the resident server (wc_k_serve:
    no launch per call) are exact for both kinds over every start phase and
    length up to the server's 4064-B limit (and past it: the launch path),
    batches larger than the wave count (several packets per wave) included;
    the server stops when idle and restarts on the next call."""
    import time
    monkeypatch.setenv("WC_SERVE_WAVES", waves)
    monkeypatch.setenv("WC_SERVE_MAX", "1024")
    wc.reload_config()
    rng = np.random.default_rng(int(waves))
    slot = 8192
    pool = rng.integers(0, 256, 512 * slot, dtype=np.uint8)
    wc.host_register(pool)
    s0 = wc.server_stats()
    try:
        for n in (1, 2, 7, 64, 65, 300, 1024):
            for kind in ("ip", "payload"):
                slots = rng.permutation(512)[: min(n, 512)]
                slots = np.resize(slots, n)  # n > 512: slots reused (overlap is fine)
                offs = (slots.astype(np.uint64) * slot + rng.integers(0, 16, n).astype(np.uint64))
                lens = rng.integers(0, 4065, n).astype(np.uint16)
                lens[: min(n, 4)] = [0, 1, 4064, 4063][: min(n, 4)]
                if n == 7:
                    lens[6] = 4065  # past the server's limit: the launch path
                if kind == "payload":
                    pkts = random_packets(rng, n, max_payload=3000, wild=True)
                    for o, (p, ln) in zip(offs, pkts):
                        pool[int(o): int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
                    lens = np.array([ln for _, ln in pkts], dtype=np.uint16)
                k = 0 if kind == "ip" else 1
                want = c_oracle.cksum_ragged(pool, offs, lens, kind=k)
                got = wc.cksum_host(pool, offs, lens, kind=kind)
                np.testing.assert_array_equal(got, want, err_msg=f"n={n} {kind}")
        time.sleep(0.1)  # idle: the watcher stops the grid
        torch.cuda.synchronize()
        offs = np.arange(64, dtype=np.uint64) * slot + 5
        lens = np.full(64, 1472, dtype=np.uint16)
        np.testing.assert_array_equal(wc.cksum_host(pool, offs, lens),
                                      c_oracle.cksum_ragged(pool, offs, lens))
        s1 = wc.server_stats()
        # every batch (14 in the loop, the one after the idle stop) but the
        # ip_cksum n = 7 one (a packet past 4064 B: the launch path) was
        # answered by the server, none fell back; idle stop + restart = a
        # second grid launch at least
        assert s1["served"] - s0["served"] == 14, (s0, s1)
        assert s1["fallbacks"] == s0["fallbacks"], (s0, s1)
        assert s1["launches"] - s0["launches"] >= 2, (s0, s1)
    finally:
        wc.host_unregister(pool)
        monkeypatch.delenv("WC_SERVE_WAVES")
        monkeypatch.delenv("WC_SERVE_MAX")
        wc.reload_config()


def test_host_server_grid_holds_up_no_other_stream(gpu, monkeypatch):
    """While the resident grid runs, work on other streams is not queued
    behind it: HIP shares a few hardware queues among a process's streams,
    and a command behind the never-ending grid on the same queue would wait
    for it to leave (up to its 4-s drain, the idle watcher being held off
    here).  With the grid up: a device batch on each of 12 new streams, each
    synchronised on its stream alone, the zero-copy launch path (a batch past
    the server's size) and the scalar drop-in all finish at once, and the grid
    is still the same one afterwards (no relaunch)."""
    import time
    monkeypatch.setenv("WC_SERVE_IDLE_US", "30000000")  # the watcher stays out of it
    wc.reload_config()
    rng = np.random.default_rng(78)
    slot = 2048
    pool = rng.integers(0, 256, 2048 * slot, dtype=np.uint8)
    wc.host_register(pool)
    try:
        one_off = np.array([5], dtype=np.uint64)
        one_len = np.array([700], dtype=np.uint16)
        want1 = c_oracle.cksum_ragged(pool, one_off, one_len)
        np.testing.assert_array_equal(wc.cksum_host(pool, one_off, one_len), want1)  # grid up
        s0 = wc.server_stats()
        n, L = 4096, 1472
        buf = torch.empty(n * L + 64, dtype=torch.uint8, device=gpu)
        wc.synth_fill(buf, 9, nbytes=n * L)
        streams = [torch.cuda.Stream(device=gpu) for _ in range(12)]
        outs = [torch.empty(n, dtype=torch.uint16, device=gpu) for _ in streams]
        torch.cuda.current_stream(gpu).synchronize()  # (the fill; a stream sync)
        t0 = time.monotonic()
        for st, o in zip(streams, outs):
            wc.cksum_strided(buf, L, L, n, out=o, stream=st)
        for st in streams:
            st.synchronize()
        dt_dev = time.monotonic() - t0
        want = c_oracle.cksum_strided(buf[: n * L].cpu().numpy(), L, L, n)
        for o in outs:
            np.testing.assert_array_equal(o.cpu().numpy(), want)
        offs = (np.arange(1500, dtype=np.uint64) * slot + 3).astype(np.uint64)
        lens = rng.integers(0, 1500, 1500).astype(np.uint16)
        t1 = time.monotonic()
        got = wc.cksum_host(pool, offs, lens)  # > WC_SERVE_MAX: the zero-copy launch
        dt_zc = time.monotonic() - t1
        np.testing.assert_array_equal(got, c_oracle.cksum_ragged(pool, offs, lens))
        pkt = pool[:1200].copy()
        t2 = time.monotonic()
        assert wc.ip_cksum(pkt) == c_oracle.ip_cksum(pkt)
        dt_sc = time.monotonic() - t2
        np.testing.assert_array_equal(wc.cksum_host(pool, one_off, one_len), want1)
        s1 = wc.server_stats()
        assert dt_dev < 0.5 and dt_zc < 0.5 and dt_sc < 0.5, (dt_dev, dt_zc, dt_sc)
        assert s1["served"] - s0["served"] == 1, (s0, s1)
        assert (s1["fallbacks"], s1["launches"]) == (s0["fallbacks"], s0["launches"]), (s0, s1)
    finally:
        wc.host_unregister(pool)
        monkeypatch.delenv("WC_SERVE_IDLE_US")
        wc.reload_config()


def test_host_server_light_traffic_then_full_batch(gpu, monkeypatch):
    """under steady light traffic (1-packet calls, every
    other wave never sees a request) past the grid's own 4-s drain time, a
    batch that needs every wave is still answered by the server -- no wave
    left on its own clock (the heartbeat keeps the grid whole), no fallback,
    no relaunch.  Then a grid left idle past half its drain time (the idle
    watcher held off) is restarted by the next call, not half-used."""
    import time
    monkeypatch.setenv("WC_SERVE_WAVES", "64")
    monkeypatch.setenv("WC_SERVE_IDLE_US", "30000000")  # the watcher stays out of it
    wc.reload_config()
    rng = np.random.default_rng(77)
    slot = 2048
    pool = rng.integers(0, 256, 256 * slot, dtype=np.uint8)
    wc.host_register(pool)
    try:
        one_off = np.array([3], dtype=np.uint64)
        one_len = np.array([1472], dtype=np.uint16)
        want1 = c_oracle.cksum_ragged(pool, one_off, one_len)
        wc.cksum_host(pool, one_off, one_len)  # starts the grid
        s0 = wc.server_stats()
        t0 = time.monotonic()
        calls = 0
        while time.monotonic() - t0 < 4.6:  # past kSrvSafetyMs (4 s)
            np.testing.assert_array_equal(wc.cksum_host(pool, one_off, one_len), want1)
            calls += 1
            time.sleep(0.002)
        offs = (np.arange(200, dtype=np.uint64) * slot + 7).astype(np.uint64)
        lens = rng.integers(0, 2000, 200).astype(np.uint16)
        want = c_oracle.cksum_ragged(pool, offs, lens)
        t1 = time.monotonic()
        np.testing.assert_array_equal(wc.cksum_host(pool, offs, lens), want)
        assert time.monotonic() - t1 < 0.5  # answered at once, no 50-ms / 2-s wait
        s1 = wc.server_stats()
        assert s1["served"] - s0["served"] == calls + 1, (s0, s1)
        assert (s1["fallbacks"], s1["launches"]) == (s0["fallbacks"], s0["launches"]), (s0, s1)
        time.sleep(2.3)  # idle past half the drain time: the next call restarts it
        np.testing.assert_array_equal(wc.cksum_host(pool, offs, lens), want)
        s2 = wc.server_stats()
        assert s2["served"] - s1["served"] == 1 and s2["fallbacks"] == s1["fallbacks"], (s1, s2)
        assert s2["launches"] - s1["launches"] == 1, (s1, s2)
    finally:
        wc.host_unregister(pool)
        monkeypatch.delenv("WC_SERVE_WAVES")
        monkeypatch.delenv("WC_SERVE_IDLE_US")
        wc.reload_config()


def test_host_server_pause_bounds_device_sync(gpu):
    """VERDICT r05 item 5.  Under steady small-batch traffic (one thread
    issuing 1-packet registered calls back to back -- the RX drain of
    backend_netmap.c:379-391) the resident grid never goes idle, so a
    device-wide synchronisation in the same process waits as long as the
    traffic lasts: 0.4 s of traffic here, a sync issued 0.1 s in.  After
    wc_server_pause() the same sync returns at once while the traffic goes on
    (on the zero-copy launch), every result is oracle-exact, the server
    answers nothing while paused and answers again after wc_server_resume()."""
    import threading
    import time
    rng = np.random.default_rng(55)
    pool = rng.integers(0, 256, 64 * 2048, dtype=np.uint8)
    one_off = np.array([3], dtype=np.uint64)
    one_len = np.array([1472], dtype=np.uint16)
    want1 = c_oracle.cksum_ragged(pool, one_off, one_len)
    bad, calls = [], [0]
    stop = threading.Event()

    def traffic(seconds):
        t_end = time.monotonic() + seconds
        while not stop.is_set() and time.monotonic() < t_end:
            got = wc.cksum_host(pool, one_off, one_len)
            if got[0] != want1[0]:
                bad.append(int(got[0]))
            calls[0] += 1

    wc.host_register(pool)
    paused = False
    try:
        wc.cksum_host(pool, one_off, one_len)  # the grid up
        # the hazard: a sync under steady traffic lasts as long as the traffic
        th = threading.Thread(target=traffic, args=(0.4,))
        th.start()
        time.sleep(0.1)
        t0 = time.monotonic()
        torch.cuda.synchronize()
        dt_unpaused = time.monotonic() - t0
        th.join()
        # the bound: pause, then sync, while the traffic goes on
        th = threading.Thread(target=traffic, args=(30.0,))
        th.start()
        time.sleep(0.1)
        s0 = wc.server_stats()
        t0 = time.monotonic()
        wc.server_pause()
        paused = True
        dt_pause = time.monotonic() - t0
        t1 = time.monotonic()
        torch.cuda.synchronize()
        dt_sync = time.monotonic() - t1
        s1 = wc.server_stats()
        c1 = calls[0]
        time.sleep(0.2)
        s2 = wc.server_stats()
        c2 = calls[0]
        wc.server_resume()
        paused = False
        time.sleep(0.2)
        stop.set()
        th.join()
        s3 = wc.server_stats()
    finally:
        stop.set()
        if paused:
            wc.server_resume()
        wc.host_unregister(pool)
    print(f"sync under traffic {dt_unpaused * 1e3:.1f} ms; pause {dt_pause * 1e3:.2f} ms, "
          f"sync after it {dt_sync * 1e3:.2f} ms; calls while paused {c2 - c1} in 0.2 s, "
          f"served while paused {s2['served'] - s1['served']}, after resume "
          f"{s3['served'] - s2['served']}")
    assert not bad, bad[:8]
    assert dt_unpaused > 0.2, dt_unpaused  # waited for the traffic to end
    assert dt_pause < 0.05 and dt_sync < 0.05, (dt_pause, dt_sync)
    assert c2 - c1 > 100  # the traffic went on while paused ...
    assert s2["served"] - s1["served"] <= 1, (s1, s2)  # ... on the zero-copy launch
    assert s3["served"] - s2["served"] > 100, (s2, s3)  # and the server answers again
    assert s3["fallbacks"] == s0["fallbacks"], (s0, s3)
    with pytest.raises(wc.WcError):
        wc.server_resume()  # (no pause to end)


@pytest.mark.parametrize("register,serve", [(True, True), (True, False), (False, False)])
def test_host_fused_ip_udp_short_len(gpu, monkeypatch, register, serve):
    """an IPv4 header (with options) longer than `len`.  The
    reference leaves payload_cksum(pkt, len < hl) undefined (its
    `len - hl` wraps to ~4 GiB, in_cksum.c:164), but mk_ip4_hdr's header
    checksum ip_cksum(pkt, hl) is defined whatever len is: the server, the
    zero-copy launch and the pipeline all reload the header past len and
    agree with the oracle on it."""
    monkeypatch.setenv("WC_SERVE", "1" if serve else "0")
    wc.reload_config()
    rng = np.random.default_rng(7 + register + 2 * serve)
    n, slot = 96, 256
    pool = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
    offs = (np.arange(n, dtype=np.uint64) * slot + rng.integers(0, 16, n).astype(np.uint64))
    ihl = rng.integers(6, 16, n)
    lens = np.array([int(rng.integers(20, 4 * h)) for h in ihl], dtype=np.uint16)  # 20 <= len < hl
    for o, h in zip(offs.astype(np.int64), ihl):
        pool[o] = 0x40 | h
    want_h = c_oracle.cksum_ragged(pool, offs, (ihl * 4).astype(np.uint16), kind=0)
    if register:
        wc.host_register(pool)
    s0 = wc.server_stats()
    try:
        got_h, _ = wc.cksum_ip_udp_host(pool, offs, lens)
    finally:
        if register:
            wc.host_unregister(pool)
        monkeypatch.delenv("WC_SERVE")
        wc.reload_config()
    s1 = wc.server_stats()
    np.testing.assert_array_equal(got_h, want_h)
    assert s1["served"] - s0["served"] == (1 if register and serve else 0)


def test_host_register_after_free_and_reuse(gpu):
    """register -> free without unregister -> a new buffer mapped at the same
    address -> register again: the zero-copy path must read the NEW pages
    (the library re-pins on every register of a base), and a re-register of
    a live region at a larger size keeps working."""
    import ctypes
    import ctypes.util
    libc = ctypes.CDLL(ctypes.util.find_library("c"), use_errno=True)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int, ctypes.c_long]
    libc.munmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    PROT_RW, MAP_PRIV_ANON, MAP_FIXED = 0x3, 0x22, 0x10
    size, slot, n = 1 << 20, 2048, 256
    addr = libc.mmap(None, size, PROT_RW, MAP_PRIV_ANON, -1, 0)
    assert addr not in (None, ctypes.c_void_p(-1).value)
    rng = np.random.default_rng(77)
    offs = (np.arange(n, dtype=np.uint64) * slot + 3).astype(np.uint64)
    lens = rng.integers(1, slot - 8, n).astype(np.uint16)
    try:
        a1 = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(addr))
        a1[:] = rng.integers(0, 256, size, dtype=np.uint8)
        wc.host_register(a1)
        np.testing.assert_array_equal(wc.cksum_host(a1, offs, lens),
                                      c_oracle.cksum_ragged(a1, offs, lens))
        # freed without wc_host_unregister; new pages mapped at the same address
        assert libc.munmap(addr, size) == 0
        got_addr = libc.mmap(addr, size, PROT_RW, MAP_PRIV_ANON | MAP_FIXED, -1, 0)
        assert got_addr == addr
        a2 = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(addr))
        a2[:] = rng.integers(0, 256, size, dtype=np.uint8)
        wc.host_register(a2)
        want2 = c_oracle.cksum_ragged(a2, offs, lens)
        np.testing.assert_array_equal(wc.cksum_host(a2, offs, lens), want2)
        # same base, smaller then larger size: still registered, still exact
        wc.host_register(a2[: size // 2])
        np.testing.assert_array_equal(wc.cksum_host(a2, offs, lens), want2)
        wc.host_register(a2)
        np.testing.assert_array_equal(wc.cksum_host(a2, offs, lens), want2)
        wc.host_unregister(a2)
        np.testing.assert_array_equal(wc.cksum_host(a2, offs, lens), want2)  # pipelined now
    finally:
        libc.munmap(addr, size)


@pytest.mark.parametrize("kind", ["ip", "payload"])
def test_host_path_unordered_gather(gpu, kind):
    """Offsets in random order through the pipelined path (gathered into
    pinned staging), more than one 64 MiB chunk, both kinds."""
    rng = np.random.default_rng(13)
    lens = synth.zipf_lengths(400000, seed=6)
    offs = synth.packed_offsets(lens, lead=1)
    buf = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 64, dtype=np.uint8)
    perm = rng.permutation(lens.size)
    offs, lens = offs[perm], lens[perm]
    got = wc.cksum_host(buf, offs, lens, kind=kind)
    np.testing.assert_array_equal(
        got, c_oracle.cksum_ragged(buf, offs, lens, kind=0 if kind == "ip" else 1))


HANDOVER_N = 3100
# The launch path each knob set forces for 3100 registered scrambled slots:
# one zero-copy launch (<= 4096 packets, under 8 MiB); the in-place stream in
# launches of 1024, 1024, 1024 and 52 packets (1024 is the floor of
# WC_ZS_PKTS), so both buffers are used twice and the last chunk is partial;
# the pipeline's packet-by-packet gather (scrambled slots do not ascend).
HANDOVER_KNOBS = {"zero_copy": {},
                  "stream": {"WC_ZC_BYTES": "0", "WC_ZS_PKTS": "1024"},
                  "gather": {"WC_ZC_BYTES": "0", "WC_ZC_STREAM": "0"}}


@pytest.fixture(params=list(HANDOVER_KNOBS))
def handover_path(request, monkeypatch, gpu):
    knobs = HANDOVER_KNOBS[request.param]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    wc.reload_config()
    yield request.param
    for k in knobs:
        monkeypatch.delenv(k)
    wc.reload_config()


@functools.lru_cache(maxsize=None)
def handover_batch(what: str):
    """(buf, offs, lens, want) of 3100 packets or frames in scrambled 2048-B
    slots, with the oracle's results; shared by the runs and never written."""
    n, slot = HANDOVER_N, 2048
    rng = np.random.default_rng(n + len(what))
    if what == "packets":
        buf = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
        pkts = random_packets(rng, n, max_payload=slot - 100, wild=True)
        offs = (rng.permutation(n) * slot + rng.integers(0, 16, n)).astype(np.uint64)
        lens = np.array([ln for _, ln in pkts], dtype=np.uint16)
        for o, (p, _) in zip(offs, pkts):
            buf[int(o): int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
        want = {"ip": c_oracle.cksum_ragged(buf, offs, lens, kind=0),
                "payload": c_oracle.cksum_ragged(buf, offs, lens, kind=1),
                "fused": fused_want(buf, offs, lens)}
    else:
        buf, offs, lens = slot_ring(rx_ring(rng, n), rng=rng)
        if what == "tx":
            tx_model.garble_fields(buf, offs, lens, rng)
            want = tx_model.Expect(buf, offs, lens)
        else:
            want = c_oracle.rx_verdict_ragged(buf, offs, lens)
    for a in (buf, offs, lens):
        a.setflags(write=False)
    return buf, offs, lens, want


@pytest.mark.parametrize("call", ["ip", "payload", "fused", "rx", "tx"])
def test_host_every_kind_every_path(gpu, call, handover_path):
    """Every host call through every launch path, the hand-over between the
    path's buffers crossed: each result array the call returns equals the
    oracle's element for element (the seal: status codes, error count and the
    frame bytes), and the resident server is never asked (n > 256)."""
    what = {"rx": "rx", "tx": "tx"}.get(call, "packets")
    shared, offs, lens, want = handover_batch(what)
    buf = shared.copy()
    wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        if call in ("ip", "payload"):
            got = [wc.cksum_host(buf, offs, lens, kind=call)]
            want = [want[call]]
        elif call == "fused":
            got, want = wc.cksum_ip_udp_host(buf, offs, lens), want["fused"]
        elif call == "rx":
            got = wc.rx_verdict_host(buf, offs, lens)
            want = (want, int(np.isin(want, wc.RX_DROPS).sum()))
        else:
            got, want = wc.tx_seal_host(buf, offs, lens), (want.status, want.errors, want.buf)
    finally:
        wc.host_unregister(buf)
    assert wc.server_stats() == s0
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    if call == "tx":
        assert_same_bytes(buf, want[2], f"host seal, {handover_path}")
    else:
        assert_same_bytes(buf, shared, f"{call} must not write the packets")


def test_host_fused_pipeline_slot_reuse(gpu):
    """3 * 2^20 + 64 minimal IPv4/UDP packets (28 bytes: IHL 5, an 8-byte UDP
    header, no payload) back to back in pageable memory: the pipeline's range
    copy in four chunks of at most 2^20 packets, the fourth in slot 0 again
    with both result arrays in play.  (hl == len - 8: len >= hl, inside
    payload_cksum's defined inputs.)"""
    n = 3 * 2**20 + 64
    rng = np.random.default_rng(28)
    pk = rng.integers(0, 256, (n, 28), dtype=np.uint8)  # tos, id, ttl, addresses, ports: random
    pk[:, 0] = 0x45
    pk[:, 2:4] = (0, 28)        # total length
    pk[:, 6:8] = (0x40, 0)      # DF
    pk[:, 9] = 17
    pk[:, 10:12] = 0            # header checksum
    pk[:, 24:26] = (0, 8)       # UDP length
    pk[:, 26:28] = 0            # UDP checksum
    buf = pk.reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * 28
    lens = np.full(n, 28, dtype=np.uint16)
    want_h, want_p = fused_want(buf, offs, lens)
    got_h, got_p = wc.cksum_ip_udp_host(buf, offs, lens)
    np.testing.assert_array_equal(got_h, want_h)
    np.testing.assert_array_equal(got_p, want_p)


def test_host_path_rejects_out_of_range(gpu):
    buf = np.zeros(4096, dtype=np.uint8)
    with pytest.raises(wc.WcError):
        wc.cksum_host(buf, np.array([4000], dtype=np.uint64), np.array([200], dtype=np.uint16))
    with pytest.raises(wc.WcError):  # payload_cksum reads >= 20 header bytes
        wc.cksum_host(buf, np.array([4090], dtype=np.uint64), np.array([4], dtype=np.uint16),
                      kind="payload")


def test_c_dropin_program(gpu, tmp_path):
    """A C caller linking libwccksum.so in place of in_cksum.c."""
    exe = tmp_path / "dropin"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c" / "dropin_test.c"), "-o", str(exe),
                    f"-L{ROOT / 'warpcore_amd'}", "-lwccksum", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{ROOT / 'warpcore_amd'}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dropin: ok" in r.stdout


def test_c_multi_gpu_program(gpu, tmp_path):
    """A single-threaded C host driving the multi-GPU ABI (tests/c/multi_test.c):
    wc_cksum_host_multi over every visible GPU and over 4 shards sharing
    cuda:0, device-resident shards and the RCCL result gather, all against
    the oracle."""
    exe = tmp_path / "multi_test"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{ROOT / 'oracle'}",
                    str(ROOT / "tests" / "c" / "multi_test.c"), str(ROOT / "oracle" / "wc_oracle.c"),
                    "-o", str(exe), f"-L{ROOT / 'warpcore_amd'}", "-lwccksum",
                    "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
                    f"-Wl,-rpath,{ROOT / 'warpcore_amd'}"], check=True)
    r = subprocess.run([str(exe), "300000"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "multi: ok" in r.stdout


@pytest.mark.parametrize("kind", ["ip", "payload"])
def test_host_multi_python(gpu, kind):
    """The Python mirror of the multi-GPU host path: 3 shards sharing cuda:0,
    wild IPv4/IPv6 packets, registered and pageable; then one shard per
    visible GPU and the RCCL gather of device-resident shard results."""
    rng = np.random.default_rng(31)
    pkts = random_packets(rng, 60000, max_payload=1472, wild=True)
    buf, offs, lens = pack(pkts, align=1, lead=7)
    want = c_oracle.cksum_ragged(buf, offs, lens, kind=0 if kind == "ip" else 1)
    try:
        assert wc.gpu_init_multi(devices=[0, 0, 0]) == 3
        np.testing.assert_array_equal(wc.cksum_host_multi(buf, offs, lens, kind=kind), want)
        wc.host_register(buf)
        try:
            np.testing.assert_array_equal(wc.cksum_host_multi(buf, offs, lens, kind=kind), want)
        finally:
            wc.host_unregister(buf)
        G = wc.gpu_init_multi()
        devs = [torch.device("cuda", g) for g in range(G)]
        bases, o_s, l_s, outs, counts = [], [], [], [], []
        for g, dv in enumerate(devs):
            lo, hi = wc.shard_range(lens.size, g, G)
            b0 = int(offs[lo])
            b1 = int(offs[hi - 1]) + max(int(lens[hi - 1]), 20)
            bases.append(dev_u8(buf[b0:b1], dv))
            o_s.append(to_dev((offs[lo:hi] - np.uint64(b0)).astype(np.uint64), dv))
            l_s.append(to_dev(lens[lo:hi], dv))
            outs.append(torch.empty(hi - lo, dtype=torch.uint16, device=dv))
            counts.append(hi - lo)
        wc.cksum_ragged_multi(bases, o_s, l_s, outs, kind=kind)
        alls = [torch.empty(lens.size, dtype=torch.uint16, device=dv) for dv in devs]
        wc.gather_results_multi(outs, counts, alls)
        for a in alls:
            torch.cuda.synchronize(a.device)
            np.testing.assert_array_equal(host(a), want)
    finally:
        wc._lib.load().wc_gpu_fini()
        wc.gpu_init(0)


def build_sock_verify(out: Path) -> Path:
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{ROOT / 'oracle'}",
                    str(ROOT / "tests" / "c" / "sock_verify.c"), str(ROOT / "oracle" / "wc_oracle.c"),
                    "-o", str(out), f"-L{ROOT / 'warpcore_amd'}", "-lwccksum",
                    "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
                    f"-Wl,-rpath,{ROOT / 'warpcore_amd'}"], check=True)
    return out


@pytest.mark.parametrize("batch,length", [(1, 1472), (64, 1472), (7, 1)])
def test_socket_rx_verify_pass(gpu, tmp_path, batch, length):
    """SURVEY config 1 with the verify pass on the socket RX path (8(f) row
    4): echo over loopback, every received payload checksummed by the GPU in
    place from the registered pool and matched against TX and the oracle."""
    exe = build_sock_verify(tmp_path / "sock_verify")
    r = subprocess.run([str(exe), "-s", str(length), "-b", str(batch), "-l", "200",
                        "-t", str(tmp_path / "ping")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["gpu_mismatch"] == 0 and res["oracle_mismatch"] == 0
    assert res["packets_verified"] >= 50 * batch
    # sockping's TSV (bin/ping.c:215, 301-302), one row per round trip
    for v in ("off", "on"):
        rows = (tmp_path / f"ping.{v}.tsv").read_text().splitlines()
        assert rows[0] == "iface\tdriver\tmbps\tbyte\tpkts\ttx\trx"
        assert len(rows) == 1 + 100
        for row in rows[1:]:
            f = row.split("\t")
            assert f[:3] == ["lo", "lo", "4294967295"] and len(f) == 7
            assert f[6] == "NA" or (int(f[3]) == length and int(f[4]) == batch and int(f[6]) > 0)


# ---------------------------------------------------------------------------
# Fused IPv4 header + UDP checksum pass.

def _ip_hdr_expect(buf: np.ndarray, offs, lens) -> np.ndarray:
    b = buf.tobytes()
    return np.array([py_oracle.ip_hdr_cksum(b[int(o):int(o) + 64]) for o in offs], np.uint16)


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("align,lead", [(1, 0), (2, 14), (16, 0), (1, 5)])
def test_fused_ip_udp_ragged(gpu, monkeypatch, align, lead, mode):
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(200 + align + lead)
    pkts = random_packets(rng, 2500, max_payload=1472, wild=True)
    buf, offs, lens = pack(pkts, align=align, lead=lead)
    hdr, pay = wc.cksum_ip_udp_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu))
    np.testing.assert_array_equal(host(pay), c_oracle.cksum_ragged(buf, offs, lens, kind=1))
    np.testing.assert_array_equal(host(hdr), _ip_hdr_expect(buf, offs, lens))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
@pytest.mark.parametrize("align", [1, 2])
def test_fused_ip_udp_malformed(gpu, monkeypatch, align, mode):
    """The fused pass over random bytes read as IP packets (every IHL, both
    versions, len == hl) in packed tiles and netmap-like uniform slots: both
    checksums of every packet against the oracle."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(41 + align)
    pkts = []
    for i in range(3000):
        ln = int(rng.integers(0, 120)) if i % 3 else int(rng.integers(1000, 1501))
        b = bytearray(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
        b[0] = (0x40 | int(rng.integers(0, 16))) if rng.random() < 0.6 else (0x60 | 5)
        hl = (b[0] & 15) * 4 if b[0] >> 4 == 4 else 40
        ln = max(ln, hl)  # len < hl: the reference reads ~4 GiB (undefined)
        pkts.append((bytes(b) + rng.integers(0, 256, max(ln, 40) - 40, dtype=np.uint8).tobytes(),
                     ln))
    buf, offs, lens = pack(pkts, align=align, lead=3)
    hdr, pay = wc.cksum_ip_udp_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu))
    np.testing.assert_array_equal(host(pay), c_oracle.cksum_ragged(buf, offs, lens, kind=1))
    np.testing.assert_array_equal(host(hdr), _ip_hdr_expect(buf, offs, lens))
    # the same packets spread over 2048-B slots at +14 (uniform-length tiles)
    big = [(p, l) for p, l in pkts if l >= 1000]
    slots = np.zeros(len(big) * 2048 + 64, np.uint8)
    so = np.arange(len(big), dtype=np.uint64) * 2048 + 14
    for (pk, _), o in zip(big, so.tolist()):
        slots[o:o + len(pk)] = np.frombuffer(pk, np.uint8)
    sl = np.array([l for _, l in big], np.uint16)
    hdr, pay = wc.cksum_ip_udp_ragged(dev_u8(slots, gpu), to_dev(so, gpu), to_dev(sl, gpu))
    np.testing.assert_array_equal(host(pay), c_oracle.cksum_ragged(slots, so, sl, kind=1))
    np.testing.assert_array_equal(host(hdr), _ip_hdr_expect(slots, so, sl))


@pytest.mark.parametrize("v6", [False, True])
def test_fused_ip_udp_strided_netmap(gpu, v6):
    rng = np.random.default_rng(21 + v6)
    n, slot = 3000, 2048
    buf = np.zeros(n * slot + 64, dtype=np.uint8)
    for i in range(n):
        ihl = 5 if v6 or i % 3 else int(rng.integers(5, 16))
        plen = 1500 - 8 - (40 if v6 else 4 * ihl)
        payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        pkt, ln = ipv6_udp(payload, rng) if v6 else ipv4_udp(payload, rng, ihl=ihl)
        buf[i * slot + 14: i * slot + 14 + len(pkt)] = np.frombuffer(pkt, np.uint8)
        assert ln == 1500
    hdr, pay = wc.cksum_ip_udp_strided(dev_u8(buf, gpu), slot, 1500, n, byte_offset=14)
    offs = np.arange(n, dtype=np.uint64) * slot + 14
    np.testing.assert_array_equal(host(pay), c_oracle.cksum_strided(buf, slot, 1500, n, kind=1,
                                                                    byte_offset=14))
    np.testing.assert_array_equal(host(hdr), _ip_hdr_expect(buf, offs, None))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
def test_fused_tx_then_rx_roundtrip(gpu, monkeypatch, mode):
    """TX: header and UDP checksums computed with both fields 0 (ip4.c:184-186,
    udp.c:209-213) and stored raw; RX: the same pass over the stored packets
    gives 0 for both (ip4.c:110-115, udp.c:132-139)."""
    ragged_mode(monkeypatch, mode)
    rng = np.random.default_rng(23)
    pkts = [(p, l) for p, l in random_packets(rng, 1500, max_payload=1400, v6_share=0.3)]
    buf, offs, lens = pack(pkts, align=2, lead=14)
    d = dev_u8(buf, gpu)
    hdr, pay = wc.cksum_ip_udp_ragged(d, to_dev(offs, gpu), to_dev(lens, gpu))
    h, p = host(hdr), host(pay)
    rx = buf.copy()
    for i, o in enumerate(offs.astype(np.int64)):
        if rx[o] >> 4 == 4:
            rx[o + 10: o + 12] = np.frombuffer(int(h[i]).to_bytes(2, "little"), np.uint8)
            hl = (rx[o] & 0x0F) * 4
        else:
            hl = 40
        rx[o + hl + 6: o + hl + 8] = np.frombuffer(int(p[i]).to_bytes(2, "little"), np.uint8)
    hdr2, pay2 = wc.cksum_ip_udp_ragged(dev_u8(rx, gpu), to_dev(offs, gpu), to_dev(lens, gpu))
    p_nonzero = p != 0          # a computed 0 is sent as "no checksum" (udp.c:212)
    assert (host(hdr2) == 0).all()
    assert (host(pay2)[p_nonzero] == 0).all()


# Every path knob of the tuning build, each set to a value that would move
# the C2 / C4 / RX paths if the shipped library read it.
PATH_KNOBS = {"WC_DIAG_NOLOAD": "1", "WC_VARIANT": "64", "WC_SHAPE": "4,1,1",
              "WC_BLOCKS_PER_CU": "1", "WC_GRID": "7", "WC_SEG": "0", "WC_SEG_ROWS": "8",
              "WC_STRIDED_SEG": "2", "WC_LEAN_MAX": "0", "WC_LEAN_PHASE": "0", "WC_NT": "0",
              "WC_GATHER": "0", "WC_GRP_DENSE": "0", "WC_SPLIT_PKTS": "1000",
              "WC_SPLIT_BYTES": "4096", "WC_FLAT_UN": "1", "WC_FLAT_PK": "2",
              "WC_RX_EARLY": "1", "WC_RX_HDRT": "0", "WC_RX_SKIP": "1", "WC_RX_ADAPT": "0",
              "WC_RX_GRID": "3", "WC_ZC_BYTES": "0", "WC_RAGGED_SHAPE": "16,2,2"}


def test_production_lib_ignores_tuning_knobs(gpu, monkeypatch):
    """The shipped library reads no path knob (VERDICT r02 item 2, r05 item
    7): with every one of them set -- the result-dropping WC_VARIANT and the
    no-load WC_DIAG_NOLOAD included -- and its configuration re-read, its
    plan for C2 is the tuned table's and C2, C4 (both kinds) and an RX ring
    stay oracle-exact.  (The calls go straight to the shipped library: it is
    reloaded itself, not through wc.reload_config(), which would move them to
    the tuning build.)"""
    from warpcore_amd import _lib
    lib = _lib.load()
    assert "TUNING" not in wc.version() and not _lib.is_tuning(lib)
    for k, v in PATH_KNOBS.items():
        monkeypatch.setenv(k, v)
    assert set(PATH_KNOBS) <= set(_lib.tuning_knobs())
    lib.wc_config_reload()
    assert _lib.active() is lib
    p = wc.plan_strided(0x100000000, 1472, 1472, 1 << 20, kind="ip")
    assert (p["group"], p["chunks_per_lane"], p["unroll"], p["kernel"]) == (32, 4, 1, "group")
    n, L = 1 << 20, 1472
    d = torch.empty(n * L + 64, dtype=torch.uint8, device=gpu)
    wc.synth_fill(d, synth.SEED, nbytes=n * L)
    out = torch.full((n,), 0xABCD, dtype=torch.int32, device=gpu).to(torch.int16).view(torch.uint16)
    wc.cksum_strided(d, L, L, n, out=out)
    np.testing.assert_array_equal(host(out), c_oracle.cksum_strided(d[:n * L].cpu().numpy(), L, L, n))
    del d
    lens = synth.zipf_lengths(1 << 24)
    offs = synth.packed_offsets(lens)
    total = int(offs[-1]) + int(lens[-1])
    d = torch.empty(total + 64, dtype=torch.uint8, device=gpu)
    wc.synth_fill(d, synth.SEED, nbytes=total)
    for kind, k in (("ip", 0), ("payload", 1)):
        got = wc.cksum_ragged(d, to_dev(offs, gpu), to_dev(lens, gpu), kind=kind)
        np.testing.assert_array_equal(host(got), c_oracle.cksum_ragged(d[:total].cpu().numpy(),
                                                                       offs, lens, kind=k))
    del d
    nf = 1 << 16
    ring = torch.empty(nf * 2048 + 64, dtype=torch.uint8, device=gpu)
    wc.synth_fill(ring, synth.SEED + 5, nbytes=nf * 2048)
    f_off, f_len = synth.make_rx_ring(ring, nf, synth.zipf_lengths(nf, seed=9))
    got, _ = wc.rx_verdict_ragged(ring, to_dev(f_off, gpu), to_dev(f_len, gpu))
    np.testing.assert_array_equal(got.cpu().numpy(),
                                  c_oracle.rx_verdict_ragged(ring.cpu().numpy(), f_off, f_len))
    del ring


LEAN_LENS = [16, 32, 48, 64, 80, 96, 128, 144, 192, 256, 320, 512, 576, 768]


@pytest.mark.parametrize("length", LEAN_LENS)
@pytest.mark.parametrize("shape", ["", "4,1,2", "8,2,2", "16,3,2", "32,4,1"])
def test_lean_kernel_aligned(gpu, monkeypatch, length, shape):
    """Aligned strided batches through the lean kernel (wc_k_lean.hip): both
    kinds, tail waves (n not a multiple of a wave's packets), packets that do
    not fill their group's pass, and payload_cksum over well-formed IPv4 /
    IPv6 UDP headers, IPv4 options, IHL < 5 and random header bytes (the
    lanes recomputed exactly)."""
    for k in ("WC_SHAPE", "WC_STRIDED_SEG", "WC_LEAN_MAX"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WC_LEAN_MAX", "64")
    if shape:
        monkeypatch.setenv("WC_SHAPE", shape)
    wc.reload_config()
    G, C, U = (int(x) for x in shape.split(",")) if shape else (0, 0, 0)
    if shape and length // 16 > G * C:
        pytest.skip("shape does not cover the packet in one pass")
    rng = np.random.default_rng(length + 7 * G + C)
    for stride in (length, length + 16, 2048):
        for n in (1, 63, 1000 + G):
            buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
            d = dev_u8(buf, gpu)
            if wc.plan_strided(d.data_ptr(), stride, length, n)["kernel"] != "lean":
                assert not shape  # a forced shape always runs lean; the planner
                pytest.skip("no lean shape fills this length's pass")  # picks only filling ones
            got = host(wc.cksum_strided(d, stride, length, n, kind="ip"))
            np.testing.assert_array_equal(got, c_oracle.cksum_strided(buf, stride, length, n),
                                          err_msg=f"ip stride {stride} n {n}")
            if length < 48:
                continue
            hb = buf.copy()
            for i in range(n):
                o = i * stride
                r = i % 5
                if r == 4:  # random bytes as the header, IHL kept within len
                    b0 = int(hb[o])
                    if b0 >> 4 == 4 and (b0 & 15) * 4 > length:
                        hb[o] = 0x40 | (length // 4 & 15)
                    continue
                pl = rng.integers(0, 256, max(0, length - 48), dtype=np.uint8).tobytes()
                if r == 0:
                    pkt, _ = ipv6_udp(pl + bytes(max(0, 48 - 48)), rng)
                elif r == 1:
                    pkt, _ = ipv4_udp(pl + bytes(20), rng, ihl=int(rng.integers(6, 11)))
                elif r == 2:
                    pkt, _ = ipv4_udp(pl + bytes(20), rng)
                    pkt = bytes([0x40 | int(rng.integers(0, 5))]) + pkt[1:]
                else:
                    pkt, _ = ipv4_udp(pl + bytes(20), rng)
                pkt = pkt[:length]
                hb[o:o + len(pkt)] = np.frombuffer(pkt, np.uint8)
            d = dev_u8(hb, gpu)
            assert wc.plan_strided(d.data_ptr(), stride, length, n,
                                   kind="payload")["kernel"] == "lean"
            got = host(wc.cksum_strided(d, stride, length, n, kind="payload"))
            np.testing.assert_array_equal(got, c_oracle.cksum_strided(hb, stride, length, n,
                                                                      kind=1),
                                          err_msg=f"payload stride {stride} n {n}")
            out, bad = wc.verify_strided(d, stride, length, n, kind="payload")
            assert int(bad.item()) == int((c_oracle.cksum_strided(hb, stride, length, n,
                                                                  kind=1) != 0).sum())
