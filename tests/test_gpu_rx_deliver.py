"""RX delivery on the GPU (wc_rx_deliver_ragged / wc_rx_deliver_host /
wc_rx_select): verdicts and drop count against the C oracle, all 16 bytes of
every record and the delivered-frame list against tests/rx_deliver_model.py --
every comparison bit-exact.

A frame's verdict and record depend on its bytes alone, not on where it lies,
so one expectation per frame list is computed once and shared by every layout
and kernel mode that list is run in.
"""
import subprocess

import numpy as np
import pytest
import torch

import rx_deliver_model as model
import warpcore_amd as wc
from oracle import c_oracle
from packets import RX_CASES, eth_frame, finish_udp, ipv4_udp, ipv6_udp, pack, rx_ring, slot_ring

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def sentinel_list(n: int, d) -> torch.Tensor:
    return dev(np.full(max(n, 1), SENTINEL, np.uint32).view(np.int32), d)


class Frames:
    """A frame list and what every call on it must return."""

    def __init__(self, frames):
        self.frames = frames
        buf, offs, lens = pack(frames)
        self.exp = model.Expect(buf, offs, lens)


def run_deliver(buf, offs, lens, exp, d, want_list=True):
    """One wc_rx_deliver_ragged call checked against `exp`; the buffer ends
    64 bytes after the copied frames (nothing past a frame may be needed)."""
    n = len(offs)
    t = torch.zeros(buf.size + 64, dtype=torch.uint8, device=d)
    t[:buf.size] = dev(buf, d)
    lst = sentinel_list(n, d)
    v, rec, got_list, cnt, drops = wc.rx_deliver_ragged(
        t, dev(offs, d), dev(lens, d), want_list=want_list, out_list=lst if want_list else None)
    v = v.cpu().numpy()
    bad = np.flatnonzero(v != exp.verdicts)
    assert bad.size == 0, (f"{bad.size} verdicts differ, first {bad[:8]}: got {v[bad[:8]]} "
                           f"want {exp.verdicts[bad[:8]]}")
    assert int(drops.item()) == exp.drops
    rec = rec.cpu().numpy().reshape(-1).view(wc.RX_RECORD)
    bad = np.flatnonzero(rec != exp.records)
    assert bad.size == 0, (f"{bad.size} records differ, first {bad[:4]} (verdicts "
                           f"{exp.verdicts[bad[:4]]}): got {rec[bad[:4]]} want {exp.records[bad[:4]]}")
    if want_list:
        c = int(cnt.item())
        got = got_list.cpu().numpy().view(np.uint32)
        assert c == exp.list.size
        np.testing.assert_array_equal(got[:c], exp.list)
        assert (got[c:] == SENTINEL).all(), "entries past the count were written"
    else:
        assert got_list is None and cnt is None


# --- mixed-case rings -------------------------------------------------------

RX_MODES = {"default": {}, "ht": {"WC_RX_ADAPT": "0"}, "early": {"WC_RX_EARLY": "1"},
            "adapt_ht": {"WC_RX_FORCE": "1"}, "adapt_early": {"WC_RX_FORCE": "2"},
            "grid4": {"WC_RX_GRID": "4"}, "grid4_early": {"WC_RX_GRID": "4", "WC_RX_EARLY": "1"},
            # the instantiations with temporal stream loads (NT = false), HT and EARLY,
            # with and without the tally
            "nt0": {"WC_NT": "0"}, "nt0_ht": {"WC_NT": "0", "WC_RX_ADAPT": "0"},
            "nt0_early": {"WC_NT": "0", "WC_RX_EARLY": "1"},
            "nt0_adapt_early": {"WC_NT": "0", "WC_RX_FORCE": "2"}}


@pytest.fixture(params=list(RX_MODES))
def rx_mode(request, monkeypatch, gpu):
    """The kernel modes a deliver launch can take (HT or EARLY, fixed or by
    ADAPT with the decision pinned, a capped grid): the same results in all."""
    for k, v in RX_MODES[request.param].items():
        monkeypatch.setenv(k, v)
    wc.reload_config()
    yield request.param
    for k in RX_MODES[request.param]:
        monkeypatch.delenv(k)
    wc.reload_config()


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(11)
    m = Frames(rx_ring(rng, 30 * len(RX_CASES)))
    # OK and OK_NO_CKSUM records, and BAD_UDP_CKSUM frames: the parse has
    # their record written before the UDP sum takes it back
    assert {wc.RX_OK, wc.RX_OK_NO_CKSUM, wc.RX_BAD_UDP_CKSUM} <= set(m.exp.verdicts.tolist())
    assert set(np.unique(m.exp.verdicts).tolist()) == set(range(10))
    return m


def test_deliver_netmap_ring(gpu, mixed, rx_mode):
    buf, offs, lens = slot_ring(mixed.frames, rng=np.random.default_rng(12))
    run_deliver(buf, offs, lens, mixed.exp, gpu)


@pytest.mark.parametrize("lead", range(16))
def test_deliver_packed_every_phase(gpu, mixed, lead):
    """Frames back to back from every start phase: the port word and the UDP
    length word at every chunk phase, straddling chunk boundaries included."""
    buf, offs, lens = pack(mixed.frames, align=1, lead=lead)
    run_deliver(buf, offs, lens, mixed.exp, gpu)


def test_deliver_without_list(gpu, mixed):
    buf, offs, lens = slot_ring(mixed.frames)
    run_deliver(buf, offs, lens, mixed.exp, gpu, want_list=False)


# --- header lengths ---------------------------------------------------------

def ihl_frames(n: int):
    """IPv4 of every IHL 5..15 (the slow parse takes hl > 40) and IPv6 in turn;
    every 7th frame's UDP sum is broken, every 5th has a zero checksum."""
    rng = np.random.default_rng(n)
    out = []
    for i in range(n):
        payload = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        k = i % 12
        pkt = ipv6_udp(payload, rng)[0] if k == 11 else ipv4_udp(payload, rng, ihl=5 + k)[0]
        b = bytearray(finish_udp(pkt, zero_udp=(i % 5 == 4)))
        if i % 7 == 6:
            b[-1 if payload else (len(b) - 6)] ^= 0x04  # payload, or a port byte
        fr = eth_frame(bytes(b), rng, 0x86DD if k == 11 else 0x0800)
        out.append((fr, len(fr)))
    return out


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_deliver_every_header_length(gpu, n):
    f = Frames(ihl_frames(n))
    hls = set(f.exp.records["hl"][f.exp.records["af"] == 4].tolist())
    assert hls == set(range(20, 64, 4)) and wc.RX_BAD_UDP_CKSUM in f.exp.verdicts
    buf, offs, lens = pack(f.frames, align=1, lead=3)
    run_deliver(buf, offs, lens, f.exp, gpu)


# --- all / none accepted, n = 0, n = 1 --------------------------------------

def test_deliver_all_accepted(gpu):
    rng = np.random.default_rng(21)
    f = Frames(rx_ring(rng, 200, cases=("ok4", "ok6", "ok4opt", "nocksum"), max_payload=400))
    assert np.isin(f.exp.verdicts, (wc.RX_OK, wc.RX_OK_NO_CKSUM)).all()
    assert f.exp.list.size == 200
    run_deliver(*slot_ring(f.frames, rng=rng), f.exp, gpu)


def test_deliver_none_accepted(gpu):
    """All ARP: count 0 and the sentinel-filled list untouched."""
    rng = np.random.default_rng(22)
    f = Frames(rx_ring(rng, 130, cases=("arp",)))
    assert (f.exp.verdicts == wc.RX_NOT_IP).all() and f.exp.list.size == 0
    run_deliver(*slot_ring(f.frames, rng=rng), f.exp, gpu)


def test_deliver_empty_default_arguments(gpu):
    """An empty ring through the wrapper as a poll loop calls it: no out_list,
    the list wanted.  WC_OK, count 0, everything empty."""
    z8 = torch.zeros(64, dtype=torch.uint8, device=gpu)
    v, rec, lst, cnt, drops = wc.rx_deliver_ragged(
        z8, torch.zeros(0, dtype=torch.int64, device=gpu),
        torch.zeros(0, dtype=torch.int16, device=gpu))
    assert (v.numel(), rec.numel(), lst.numel()) == (0, 0, 0)
    assert int(cnt.item()) == 0 and int(drops.item()) == 0
    got, cnt = wc.rx_select(v, wc.RX_MASK_DELIVER)
    assert got.numel() == 0 and int(cnt.item()) == 0
    hv, hrec, hlst, hdrops = wc.rx_deliver_host(np.zeros(64, np.uint8), np.zeros(0, np.uint64),
                                                np.zeros(0, np.uint16))
    assert (hv.size, hrec.size, hlst.size, hdrops) == (0, 0, 0, 0)


def test_deliver_empty_and_single(gpu):
    z8 = torch.zeros(64, dtype=torch.uint8, device=gpu)
    lst = sentinel_list(1, gpu)
    v, rec, _, cnt, drops = wc.rx_deliver_ragged(
        z8, torch.zeros(0, dtype=torch.int64, device=gpu),
        torch.zeros(0, dtype=torch.int16, device=gpu), out_list=lst)
    assert v.numel() == 0 and rec.numel() == 0 and int(cnt.item()) == 0 and int(drops.item()) == 0
    # the empty calls write the count, they do not leave it
    from warpcore_amd import _lib
    cnt = torch.full((1,), 7, dtype=torch.int64, device=gpu)
    st = torch.cuda.current_stream(gpu).cuda_stream
    assert _lib.active().wc_rx_select(None, 0, wc.RX_MASK_DELIVER, None, cnt.data_ptr(), None,
                                      st) == 0
    assert int(cnt.item()) == 0
    cnt.fill_(7)
    assert _lib.active().wc_rx_deliver_ragged(None, None, None, 0, None, None, lst.data_ptr(),
                                              cnt.data_ptr(), None, None, st) == 0
    assert int(cnt.item()) == 0
    rng = np.random.default_rng(23)
    for case in ("ok4", "badudp", "arp"):
        f = Frames(rx_ring(rng, 1, cases=(case,), max_payload=200))
        run_deliver(*pack(f.frames, lead=7), f.exp, gpu)


# --- wc_rx_select alone ------------------------------------------------------

MASKS = (wc.RX_MASK_DELIVER, wc.RX_MASK_HOST, 0, 0xFFFFFFFF, 1 << wc.RX_BAD_UDP_CKSUM)
# One less than, equal to and one more than every granularity of the select
# kernels: the 16-byte chunk, the wave's 64 chunks (1024 B), the 256-chunk
# block (4096 B), and 1024 blocks (2^22 B), past which the one-workgroup scan
# of the block counts takes its second iteration.
SELECT_N = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 40000,
            (1 << 22) - 1, 1 << 22, (1 << 22) + 1]


def synthetic_verdicts(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 10, n, dtype=np.uint8)
    wild = rng.random(n) < 0.05
    v[wild] = rng.integers(32, 256, int(wild.sum()), dtype=np.uint8)
    if n > 3:
        v[[0, n - 1]] = (0, 1)  # the array's first and last byte match DELIVER
    return v


@pytest.mark.parametrize("n", SELECT_N)
def test_select_alone(gpu, n):
    v = synthetic_verdicts(n, n)
    # at a 16-byte boundary, and 5 bytes past one (the first chunk's head masked)
    for shift in (0, 5):
        t = torch.full((n + shift + 16,), 1, dtype=torch.uint8, device=gpu)  # would match
        t[shift:shift + n] = dev(v, gpu)
        tv = t[shift:shift + n]
        assert tv.data_ptr() % 16 == shift
        for mask in MASKS:
            want = model.select(v, mask)
            lst = sentinel_list(n, gpu)
            got, cnt = wc.rx_select(tv, mask, out=lst)
            c = int(cnt.item())
            got = got.cpu().numpy().view(np.uint32)
            assert c == want.size, (n, shift, hex(mask))
            np.testing.assert_array_equal(got[:c], want)
            assert (got[c:n] == SENTINEL).all()


def test_select_dense_and_sparse_extremes(gpu):
    """Every byte matching (each block writes a full 4096-entry run) and a
    single match in the last block."""
    n = 3 * 4096 + 100
    ones = torch.zeros(n, dtype=torch.uint8, device=gpu)
    got, cnt = wc.rx_select(ones, wc.RX_MASK_DELIVER)
    assert int(cnt.item()) == n
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), np.arange(n, dtype=np.uint32))
    v = np.full(n, wc.RX_NOT_IP, np.uint8)
    v[n - 2] = wc.RX_OK
    lst = sentinel_list(n, gpu)
    got, cnt = wc.rx_select(dev(v, gpu), wc.RX_MASK_DELIVER, out=lst)
    got = got.cpu().numpy().view(np.uint32)
    assert int(cnt.item()) == 1 and got[0] == n - 2 and (got[1:] == SENTINEL).all()


# A select block is 256 chunks of 16 verdict bytes = 4096 verdicts (kSelBlock)
# and the one-workgroup scan takes 1024 block counts per iteration (kSelScan):
# 1024 * 4096 = 2^22 verdicts per iteration, so 2^22 + 17 is the smallest
# shape with a second one (1025 blocks at offset 0, 1026 chunks' worth at
# offset 5), and 2^26 + 17 runs seventeen, the carry growing past 2^26.
SELECT_CARRY_N = [1024 * 4096 + 17, 1024 * 4096 * 16 + 17]


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("n", SELECT_CARRY_N)
def test_select_carry_across_scan_iterations(gpu, n, shift):
    """Every verdict matching -- each scan iteration adds a full 2^22 to the
    carry, and the last block's offset is the whole carry -- and exactly one
    match, in the last byte, whose offset is 0 after any number of iterations;
    at a 16-byte boundary and 5 bytes past one.  Expectations are arange(n)
    and [n - 1]; compared on the device."""
    t = torch.full((n + shift + 16,), wc.RX_OK_NO_CKSUM, dtype=torch.uint8, device=gpu)
    tv = t[shift:shift + n]  # (the bytes around it would match)
    assert tv.data_ptr() % 16 == shift
    lst = torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device=gpu)
    tv.fill_(wc.RX_NOT_IP)
    tv[n - 1] = wc.RX_OK
    got, cnt = wc.rx_select(tv, wc.RX_MASK_DELIVER, out=lst)
    assert int(cnt.item()) == 1 and int(got[0].item()) == n - 1
    assert bool((got[1:] == SENTINEL - (1 << 32)).all())
    tv.fill_(wc.RX_OK_NO_CKSUM)
    got, cnt = wc.rx_select(tv, wc.RX_MASK_DELIVER, out=lst)
    assert int(cnt.item()) == n
    assert bool((got == torch.arange(n, dtype=torch.int32, device=gpu)).all())


def test_deliver_many_frames_repeated(gpu, mixed):
    """More frames than one scan iteration's blocks cover would need real
    frames by the million; the calls only read, so 2^18 + 1 offsets point at
    the same 600 frames: several select blocks, a full grid of tiles."""
    buf, offs, lens = slot_ring(mixed.frames)
    n = (1 << 18) + 1
    idx = np.arange(n) % len(mixed.frames)
    run_deliver(buf, offs[idx], lens[idx], mixed.exp.take(idx), gpu)


# --- frames ending on the buffer's last byte --------------------------------

def test_deliver_frames_at_buffer_end(gpu):
    """One cycle of RX_CASES, each frame alone in a buffer that ends with it:
    the frame's length bounds every load, the record's fields included."""
    rng = np.random.default_rng(9)
    for fr, flen in rx_ring(rng, len(RX_CASES)):
        buf = np.frombuffer(fr[:flen], np.uint8).copy()
        t = dev(buf, gpu) if buf.size else torch.zeros(1, dtype=torch.uint8, device=gpu)
        v, rec, lst, cnt, _ = wc.rx_deliver_ragged(t, dev(np.zeros(1, np.uint64), gpu),
                                                   dev(np.array([flen], np.uint16), gpu))
        want_v = c_oracle.rx_verdict(fr, flen)
        assert int(v.item()) == want_v
        assert rec.cpu().numpy().tobytes() == model.record_of(fr, flen, want_v).tobytes()
        assert int(cnt.item()) == int(want_v in (wc.RX_OK, wc.RX_OK_NO_CKSUM))


# --- the host call ------------------------------------------------------------

@pytest.fixture(scope="module")
def host_frames():
    rng = np.random.default_rng(31)
    return Frames(rx_ring(rng, 2048, max_payload=1200))


@pytest.mark.parametrize("register", [False, True])
@pytest.mark.parametrize("n", [64, 4096, 200000])
def test_deliver_host(gpu, host_frames, register, n):
    """The ring in host memory: a zero-copy launch for a small registered
    batch, the in-place stream for a large one, the pipeline for pageable
    memory (offsets repeat over 2048 frames' slots: the call only reads).
    Never the resident server, and nothing falls back."""
    buf, offs, lens = slot_ring(host_frames.frames, rng=np.random.default_rng(n))
    idx = np.arange(n) % len(host_frames.frames)
    offs, lens = offs[idx], lens[idx]
    want_v, want_r = host_frames.exp.verdicts[idx], host_frames.exp.records[idx]
    if register:
        wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        v, rec, lst, drops = wc.rx_deliver_host(buf, offs, lens)
    finally:
        if register:
            wc.host_unregister(buf)
    s1 = wc.server_stats()
    np.testing.assert_array_equal(v, want_v)
    bad = np.flatnonzero(rec != want_r)
    assert bad.size == 0, f"{bad.size} records differ, first {bad[:4]}: {rec[bad[:4]]} vs {want_r[bad[:4]]}"
    np.testing.assert_array_equal(
        lst, np.flatnonzero(np.isin(want_v, (wc.RX_OK, wc.RX_OK_NO_CKSUM))).astype(np.uint32))
    assert drops == int(np.isin(want_v, wc.RX_DROPS).sum())
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (0, 0)


def test_deliver_host_dense_ascending(gpu, host_frames):
    """Registered, dense and ascending, too large for one zero-copy launch:
    the pipeline's range copy straight from the region."""
    frames = host_frames.frames * 4
    buf, offs, lens = pack(frames, align=1, lead=1)
    idx = np.arange(len(frames)) % len(host_frames.frames)
    wc.host_register(buf)
    try:
        v, rec, lst, drops = wc.rx_deliver_host(buf, offs, lens)
    finally:
        wc.host_unregister(buf)
    np.testing.assert_array_equal(v, host_frames.exp.verdicts[idx])
    assert (rec == host_frames.exp.records[idx]).all()
    assert lst.size == int(np.isin(v, (wc.RX_OK, wc.RX_OK_NO_CKSUM)).sum())


def test_c_rx_deliver_loop(gpu, tmp_path):
    """INTEGRATION.md section 3's deliver hook compiled in C
    (tests/c/rx_deliver_loop.c): a w_nic_rx-shaped loop that calls
    wc_rx_deliver_host, walks only h_list, fills a w_iov-shaped struct from
    each record and compares it with one filled the way udp_rx does; the
    WC_RX_MASK_HOST list is exactly the ARP / ICMP frames.  A small ring (one
    zero-copy launch) and a large one (in-place stream, pipeline)."""
    from cprog import build
    exe = build("rx_deliver_loop", tmp_path)
    for slots in ("1024", "6000"):
        r = subprocess.run([str(exe), slots], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "rx_deliver_loop: ok" in r.stdout
