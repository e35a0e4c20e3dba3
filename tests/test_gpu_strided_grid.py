"""GPU tests over tests/strided_grid.py: every case of the grid through
wc_cksum_strided (ip, payload), wc_cksum_ip_udp_strided and wc_verify_strided
in the shipped configuration (no WC_* knob), bit-exact against the C oracle;
the census that holds the grid to the planner; the lean kernel's 32-bit lane
offsets at the largest stride its guard lets through; and IPv4 headers longer
than len through both device-resident fused calls.

Parametrised by threshold: a failure names the planner threshold it stands on.
"""
import ctypes

import numpy as np
import pytest
import torch

import strided_grid as sg
import warpcore_amd as wc
from oracle import c_oracle
from packets import pack
from test_gpu_parity import RAGGED_MODES, dev_u8, fused_want, host, ragged_mode, to_dev
from warpcore_amd import _lib

pytestmark = pytest.mark.gpu

BASE = 0x100000000  # a 4-GiB-aligned address to plan at: only its phase matters
CALLS = ("ip", "payload", "fused")


def dev(buf, gpu) -> torch.Tensor:
    """dev_u8 of a grid buffer (they are shared and read-only: a copy goes up)."""
    return dev_u8(np.array(buf), gpu)


def by_buffer(cases):
    """[(the buffer's largest case, its cases)] in grid order."""
    out: dict = {}
    for c in cases:
        out.setdefault(c.group, []).append(c)
    return [(max(cs, key=lambda c: c.n), cs) for cs in out.values()]


# ---------------------------------------------------------------------------
# Parity.

@pytest.mark.parametrize("label", sg.LABELS)
def test_grid_parity(gpu, label):
    """ip_cksum, payload_cksum and the fused pair of every case standing at
    this threshold, at the case's base phase (byte_offset) in a buffer with
    dev_u8's padding; the fused call's expectation is fused_want's."""
    ran = 0
    for top, cases in by_buffer(sg.for_threshold(label)):
        buf = sg.buffer(top)
        d = dev(buf, gpu)
        want = sg.expect(top)
        if "fused" in top.kinds:  # the definition, once per buffer
            hdr, pay = fused_want(buf, top.offs, np.full(top.n, top.length, np.uint16))
            np.testing.assert_array_equal(hdr, want["hdr"])
            np.testing.assert_array_equal(pay, want["payload"])
        for c in cases:
            what = f"len {c.length} stride {c.stride} phase {c.phase} n {c.n}"
            got = host(wc.cksum_strided(d, c.stride, c.length, c.n, kind="ip",
                                        byte_offset=c.phase))
            np.testing.assert_array_equal(got, want["ip"][:c.n], err_msg="ip " + what)
            if "payload" not in c.kinds:
                continue
            got = host(wc.cksum_strided(d, c.stride, c.length, c.n, kind="payload",
                                        byte_offset=c.phase))
            np.testing.assert_array_equal(got, want["payload"][:c.n], err_msg="payload " + what)
            hdr, pay = wc.cksum_ip_udp_strided(d, c.stride, c.length, c.n, byte_offset=c.phase)
            np.testing.assert_array_equal(host(pay), want["payload"][:c.n],
                                          err_msg="fused payload " + what)
            np.testing.assert_array_equal(host(hdr), want["hdr"][:c.n],
                                          err_msg="fused header " + what)
            ran += 1
    assert ran > 100


@pytest.mark.parametrize("label", sg.LABELS)
def test_grid_verify(gpu, label):
    """wc_verify_strided on the same cases, both kinds: the results, and the
    count of non-zero checksums, which two calls into one counter add up."""
    counted = 0
    for top, cases in by_buffer(sg.for_threshold(label)):
        d = dev(sg.buffer(top), gpu)
        want = sg.expect(top)
        for c in cases:
            for kind in ("ip", "payload"):
                if kind not in c.kinds:
                    continue
                w = want[kind][:c.n]
                nz = int(np.count_nonzero(w))
                bad = torch.zeros(1, dtype=torch.int64, device=gpu)
                out, _ = wc.verify_strided(d, c.stride, c.length, c.n, kind=kind,
                                           byte_offset=c.phase, bad=bad)
                out2, bad2 = wc.verify_strided(d, c.stride, c.length, c.n, kind=kind,
                                               byte_offset=c.phase, bad=bad)
                what = f"{kind} len {c.length} stride {c.stride} phase {c.phase} n {c.n}"
                assert bad2 is bad and int(bad.item()) == 2 * nz, what
                np.testing.assert_array_equal(host(out), w, err_msg=what)
                np.testing.assert_array_equal(host(out2), w, err_msg=what)
                counted += nz
    assert counted > 1000  # the expected counts are not 0


# ---------------------------------------------------------------------------
# Census: the grid against the planner.

def _planner():
    """-> plan(call, phase, stride, length, n) = (family, G, CPL, U, FULL)."""
    lib = _lib.active()
    v = [ctypes.c_int() for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]

    def plan(call, phase, stride, length, n):
        base = BASE + phase
        if call == "fused":
            fam = lib.wc_plan_strided_fused(base, stride, length, n, *refs)
        else:
            k = wc.KIND_IP if call == "ip" else wc.KIND_PAYLOAD
            assert lib.wc_plan_strided(base, stride, length, n, k, *refs) == 0
            fam = lib.wc_plan_strided_kernel(base, stride, length, n, k)
        full = call == "ip" and base % 16 == 0 and stride % 16 == 0 and length % 16 == 0
        return fam.decode(), v[0].value, v[1].value, v[2].value, full
    return plan


# k = 1..600 in full; above it (nch > 600: past the last threshold, 576, at
# any phase) every 16th and the two ends: 0.6 million plans, about a second;
# the full sweep is 3.3 million
SWEEP_K = tuple(range(1, 601)) + tuple(range(616, 4095, 16)) + (4095, 4096)


@pytest.fixture(scope="module")
def reachable(gpu):
    plan = _planner()
    reach = {call: set() for call in CALLS}
    for k in SWEEP_K:
        for length in (16 * k - 1, 16 * k, 16 * k + 1):
            if length > 0xFFFF:
                continue
            for phase in sg.PHASES:
                for call in CALLS:
                    nch = sg.chunks(length, phase, call != "ip")
                    for stride in sg.strides_for(length, nch):
                        for n in (37, 1 << 20):
                            reach[call].add(plan(call, phase, stride, length, n))
    return reach


@pytest.mark.parametrize("call", CALLS)
def test_census_grid_hits_every_reachable_plan(gpu, reachable, call):
    """Every (kernel family, G, CPL, U, FULL) that the planner returns over
    lens 16k - 1, 16k, 16k + 1 (k = 1..4096, thinned above 600), the grid's
    phases and stride classes, n = 37 and 2^20, is the plan of at least one
    grid case of this call: none is exempt.

    Sizes of the reachable sets: ip 35 (27 group, 6 lean, 2 seg), payload 22
    (14 group, 7 lean, 1 seg), fused 14 (group only: the header pass takes
    neither the seg nor the lean route)."""
    plan = _planner()
    hit = {plan(call, c.phase, c.stride, c.length, c.n)
           for c in sg.grid() if call == "ip" or call in c.kinds}
    reach = reachable[call]
    print(f"{call}: {len(reach)} reachable plans, {len(hit)} hit by the grid")
    assert len(reach) == {"ip": 35, "payload": 22, "fused": 14}[call], sorted(reach)
    assert not reach - hit, f"no grid case runs {sorted(reach - hit)}"
    if call == "fused":
        assert {p[0] for p in reach | hit} == {"group"}
        # the eleven HDR instances that nothing ran before the grid, and the three that did
        assert {p[1:4] for p in reach} == {
            (4, 2, 2), (8, 1, 4), (8, 3, 2), (16, 2, 4), (8, 6, 1), (16, 3, 2), (16, 5, 4),
            (32, 4, 1), (64, 4, 1), (32, 18, 1), (64, 9, 1), (4, 1, 4), (16, 6, 2), (32, 3, 2)}
    else:
        assert {p[0] for p in reach} == {"group", "lean", "seg"}


def test_fused_plan_is_the_payload_plan_without_seg_and_lean(gpu):
    """wc.plan_strided(fused=True) where the payload plan is overwritten:
    packed 576 B (seg), aligned 256 B (lean), 128 B in slots at +14 (PH)."""
    for phase, stride, length, other in ((0, 576, 576, "seg"), (0, 256, 256, "lean"),
                                         (14, 2048, 128, "lean")):
        p = wc.plan_strided(BASE + phase, stride, length, 1 << 20, kind="payload")
        f = wc.plan_strided(BASE + phase, stride, length, 1 << 20, fused=True)
        assert p["kernel"] == other and f["kernel"] == "group" and f["group"] >= 4
        assert f["grid"] >= 1 and set(f) == set(p)
    p = wc.plan_strided(BASE, 1472, 1472, 1 << 20, kind="payload")
    assert wc.plan_strided(BASE, 1472, 1472, 1 << 20, fused=True) == p  # C2: the same plan


# ---------------------------------------------------------------------------
# The lean kernel's guard: PPW * stride < 2^32 keeps its 32-bit lane offsets.

@pytest.mark.parametrize("kind", ["ip", "payload"])
def test_lean_guard_largest_stride(gpu, kind):
    """64 packets of 64 B at stride 2^26 - 16 (lean: (4,1,4), 64 packets per
    wave, 64 x stride just below 2^32) and at 2^26 (not lean).  The default
    3-GiB split makes the first launch 48 packets: lane offsets up to 47 x
    stride, above 2^31.  Only the packets and 16 bytes on either side of each
    are written; the oracle gets a compact copy."""
    n, length, guard = 64, 64, 16
    slot = guard + length + guard
    rng = np.random.default_rng([sg.SEED, 0x1EA4, kind == "ip"])
    compact = rng.integers(1, 256, n * slot, dtype=np.uint8)
    for i in range(n):  # payload: len >= hl for every header kind of the grid
        first = (0x45, 0x46 + i % 10, 0x40 + i % 5, 0x60, 0x60, 0x45)[i % 6]
        compact[i * slot + guard] = first
    k = 0 if kind == "ip" else 1
    want = c_oracle.cksum_strided(compact, slot, length, n, kind=k, byte_offset=guard)
    assert np.count_nonzero(want) > 60
    d = torch.empty((n - 1) * (1 << 26) + length + guard + 64, dtype=torch.uint8, device=gpu)
    assert d.numel() < 1 << 32 and d.data_ptr() % 16 == 0
    src = torch.from_numpy(compact).to(gpu)
    for stride, lean in (((1 << 26) - 16, True), (1 << 26, False)):
        p = wc.plan_strided(d.data_ptr(), stride, length, n, kind=kind)
        assert (p["kernel"] == "lean") == lean, (stride, p)
        if lean:
            assert (p["group"], p["chunks_per_lane"], p["unroll"]) == (4, 1, 4)
            assert 47 * stride > 1 << 31
        for i in range(n):
            lo = guard if i == 0 else 0  # nothing lies before packet 0
            d[i * stride - guard + lo:i * stride + length + guard] = \
                src[i * slot + lo:(i + 1) * slot]
        got = host(wc.cksum_strided(d, stride, length, n, kind=kind))
        np.testing.assert_array_equal(got, want, err_msg=f"stride {stride}")
    del d


# ---------------------------------------------------------------------------
# IPv4 headers longer than len (20 <= len < hl): the header checksum alone.

@pytest.mark.parametrize("length", sg.SHORT_LENS)
def test_short_header_strided(gpu, length):
    """d_out_ip_hdr[i] = ip_cksum(pkt, ip4_hl(pkt[0])) whatever len is: IHL
    cycling over every value with hl > len, every base phase, packed (the
    headers overlap the packets behind), 64-B and 2048-B strides.  While the
    HDR instances summed the header from the chunks of max(len, 20) bytes
    alone, every length of this family failed here (at len 59 only the
    packets whose header ends one chunk further than their span)."""
    cases = [c for c in sg.short_header_cases() if c.length == length]
    assert len(cases) == 60
    for c in cases:
        buf = sg.short_buffer(c)
        hdr, _ = wc.cksum_ip_udp_strided(dev(buf, gpu), c.stride, c.length, c.n,
                                         byte_offset=c.phase)
        np.testing.assert_array_equal(host(hdr), sg.short_expect(c), err_msg=str(c))


@pytest.mark.parametrize("mode", list(RAGGED_MODES))
def test_short_header_ragged(gpu, monkeypatch, mode):
    """The same family through wc_cksum_ip_udp_ragged in every ragged mode,
    each packet's bytes being its whole header."""
    ragged_mode(monkeypatch, mode)
    pkts = list(sg.short_packets())
    for align, lead in ((1, 0), (1, 5), (2, 14), (16, 0)):
        buf, offs, lens = pack(pkts, align=align, lead=lead)
        hdr, _ = wc.cksum_ip_udp_ragged(dev_u8(buf, gpu), to_dev(offs, gpu), to_dev(lens, gpu))
        np.testing.assert_array_equal(host(hdr), sg.header_checksums(buf, offs),
                                      err_msg=f"align {align} lead {lead}")
