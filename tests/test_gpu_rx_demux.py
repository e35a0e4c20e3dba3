"""RX socket demultiplex on the GPU (wc_rx_demux / wc_rx_demux_host): every
socket byte, list entry and start entry against tests/rx_demux_model.py --
bit-exact; the lists are pre-filled with a sentinel that entries past the
total must still hold.

A frame's record and socket depend on its bytes and the table alone, not on
where the frame lies, so one expectation per frame list is computed once and
shared by every layout and size that list is run in.
"""
import subprocess

import numpy as np
import pytest
import torch

import rx_deliver_model as dmodel
import rx_demux_model as model
import warpcore_amd as wc
from packets import pack, rx_ring, slot_ring
from rx_demux_cases import A4, A6, PEER4, PEER6, be16, frame_to, population, stray_frame, udp_frame

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
BLOCK = 4096  # frames per demux workgroup


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def sentinel_list(n: int, d) -> torch.Tensor:
    return dev(np.full(max(n, 1), SENTINEL, np.uint32).view(np.int32), d)


class World:
    """A socket list, a frame list, and what every call on them must return."""

    def __init__(self, socks, frames):
        self.socks, self.frames, self.ns = socks, frames, len(socks)
        self.tab = wc.rx_socktab_build(socks)
        buf, offs, lens = pack(frames)
        self.dexp = dmodel.Expect(buf, offs, lens)
        self.exp = model.Expect(model.Table(socks), frames, self.dexp.records)


def check(sock, lst, start, exp, n):
    sock = sock.cpu().numpy()
    bad = np.flatnonzero(sock != exp.sock)
    assert bad.size == 0, (f"{bad.size} socket ids differ, first {bad[:8]}: got {sock[bad[:8]]} "
                           f"want {exp.sock[bad[:8]]}")
    if lst is None:
        assert start is None
        return
    start = start.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(start, exp.start)
    got = lst.cpu().numpy().view(np.uint32)
    total = exp.list.size
    np.testing.assert_array_equal(got[:total], exp.list)
    assert (got[total:] == SENTINEL).all(), "entries past the total were written"


def run_demux(buf, offs, lens, w, exp, d, want_list=True, tight=False):
    """rx_deliver_ragged, then rx_demux behind it, checked against `exp`; the
    buffer ends 64 bytes after the copied frames, or with them (tight)."""
    n = len(offs)
    t = torch.zeros(buf.size + (0 if tight else 64), dtype=torch.uint8, device=d)
    t[:buf.size] = dev(buf, d)
    o = dev(offs, d)
    _, rec, _, _, _ = wc.rx_deliver_ragged(t, o, dev(lens, d), want_list=False)
    lst = sentinel_list(n, d) if want_list else None
    sock, got, start = wc.rx_demux(t, o, rec, dev(w.tab, d), w.ns, want_list=want_list,
                                   out_list=lst)
    check(sock, got, start, exp, n)


def mixed_frames(socks, count: int, seed: int):
    """Frames for every socket (connected ones from their remote, bound ones
    from several remotes -- a connected sibling's among them), strays no
    socket takes, IPv4 options, zero checksums, and rx_ring's frames that are
    not delivered, shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    nd = rx_ring(rng, max(count // 4, 1), max_payload=200)
    while len(out) < count - len(nd):
        k = len(out)
        if len(socks) and k % 5 != 4:
            s = socks[int(rng.integers(0, len(socks)))]
            out.append(frame_to(rng, s, ihl=5 + (k % 11 if k % 7 == 0 else 0),
                                zero_udp=(k % 13 == 0)))
        else:
            out.append(stray_frame(rng))
    out += nd
    return [out[i] for i in rng.permutation(len(out))]


@pytest.fixture(scope="module")
def world():
    socks = population(17, 1)
    w = World(socks, mixed_frames(socks, 640, 2))
    ids = set(w.exp.sock.tolist())
    assert set(range(17)) | {model.NONE, model.UNBOUND} == ids
    return w


# --- sizes and layouts --------------------------------------------------------

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, BLOCK - 1, BLOCK, BLOCK + 1, 8193,
         3 * BLOCK + 17]


@pytest.mark.parametrize("n", SIZES)
def test_demux_sizes_scrambled_slots(gpu, world, n):
    """2048-byte slots in scrambled order; the calls only read, so n offsets
    point at the same 640 frames' slots."""
    buf, offs, lens = slot_ring(world.frames, rng=np.random.default_rng(n))
    idx = (np.arange(n) * 7 + n) % len(world.frames)
    run_demux(buf, offs[idx], lens[idx], world, world.exp.take(idx), gpu)


@pytest.mark.parametrize("lead", range(16))
def test_demux_packed_every_phase(gpu, world, lead):
    """Frames back to back from every start phase: the address bytes straddle
    the 16-byte chunks every way."""
    buf, offs, lens = pack(world.frames, align=1, lead=lead)
    run_demux(buf, offs, lens, world, world.exp, gpu)


def test_demux_frame_at_buffer_end(gpu, world):
    """Frames alone in a buffer that ends with them, at every phase: no load
    may reach past the chunk of the frame's last byte."""
    rng = np.random.default_rng(3)
    frames = [udp_frame(rng, 4, A4[0], be16(4433), PEER4, be16(999), max_payload=0),
              udp_frame(rng, 6, A6[0], be16(4433), PEER6, be16(999), max_payload=0),
              udp_frame(rng, 4, A4[1], be16(53), PEER4, be16(1), max_payload=5)]
    w = World(world.socks, frames)
    assert w.exp.sock.tolist() == [1, 3, 5]
    for lead in range(16):
        for k, (fr, flen) in enumerate(frames):
            buf = np.frombuffer(bytes(lead) + fr, np.uint8).copy()
            run_demux(buf, np.array([lead], np.uint64), np.array([flen], np.uint16), w,
                      w.exp.take(np.array([k])), gpu, tight=True)


# --- socket populations -------------------------------------------------------

def test_demux_no_sockets(gpu, world):
    w = World(world.socks[:0], world.frames[:300])
    assert set(w.exp.sock.tolist()) == {model.NONE, model.UNBOUND}
    assert (w.exp.start[:255] == 0).all() and w.exp.start[255] > 0
    run_demux(*slot_ring(w.frames), w, w.exp, gpu)


def test_demux_one_socket_takes_all(gpu):
    rng = np.random.default_rng(4)
    socks = population(1, 4)
    w = World(socks, [frame_to(rng, socks[0]) for _ in range(BLOCK + 300)])
    assert (w.exp.sock == 0).all()
    run_demux(*slot_ring(w.frames, rng=rng), w, w.exp, gpu)


@pytest.mark.parametrize("half", [False, True])
def test_demux_254_sockets(gpu, half):
    """Every socket with exactly one frame; then every other socket empty."""
    rng = np.random.default_rng(5)
    socks = population(254, 5)
    order = rng.permutation(254)
    if half:
        order = np.concatenate([order[order % 2 == 0]] * 3)
    w = World(socks, [frame_to(rng, socks[i]) for i in order])
    np.testing.assert_array_equal(w.exp.sock, order.astype(np.uint8))
    run_demux(*slot_ring(w.frames, rng=rng), w, w.exp, gpu)


def test_demux_254_sockets_many_blocks(gpu):
    """255 classes over 35 blocks: 8925 counts, more than twice the 4096 the
    one-workgroup scan takes per iteration, so it runs three (and a class's
    blocks straddle two of them)."""
    rng = np.random.default_rng(11)
    socks = population(254, 11)
    frames = [frame_to(rng, socks[i]) for i in rng.permutation(254)] + \
        [stray_frame(rng) for _ in range(20)] + rx_ring(rng, 20, max_payload=100)
    w = World(socks, frames)
    n = 34 * BLOCK + 5
    assert (w.ns + 1) * (n // BLOCK + 1) > 2 * 4096
    buf, offs, lens = slot_ring(w.frames, rng=rng)
    idx = (np.arange(n) * 5 + 1) % len(frames)
    run_demux(buf, offs[idx], lens[idx], w, w.exp.take(idx), gpu)


@pytest.fixture(scope="module")
def small_v4():
    """254 bound IPv4 sockets and, in 64-byte slots, minimal frames (42 header
    bytes, up to 6 of payload) for all of them but 100..109, then strays."""
    rng = np.random.default_rng(12)
    socks = np.array([model.sock(4, A4[5], be16(6000 + i), rng=rng) for i in range(254)],
                     dtype=model.SOCK)
    to = [i for i in range(254) if not 100 <= i < 110]
    frames = [frame_to(rng, socks[i], max_payload=6) for i in to * 3] + \
        [udp_frame(rng, 4, A4[6], be16(7000 + k), PEER4, be16(9), max_payload=6) for k in range(40)]
    assert max(flen for _, flen in frames) <= 64
    return socks, frames


@pytest.mark.parametrize("ns", [254, 0])
def test_demux_scan_second_iteration(gpu, small_v4, ns):
    """n = 17 blocks + 1 frame -> 18 blocks; with 254 sockets (ns + 1) * 18 =
    4590 counts, just past the 1024 threads x 4 counts of one scan iteration,
    so the second one starts inside a class's row with the carry of the first.
    Sockets 0 and 253 and the unbound class have frames, sockets 100..109 have
    none (consecutive equal starts); the frames are drawn at random, so every
    block's counts differ.  With no socket the scan's row 0 is the unbound
    row and every delivered frame is in it."""
    socks, frames = small_v4
    w = World(socks[:ns], frames)
    n = 17 * BLOCK + 1
    assert (ns + 1) * (n // BLOCK + 1) == (4590 if ns else 18) and 4590 > 1024 * 4
    rng = np.random.default_rng(13)
    buf, offs, lens = slot_ring(w.frames, slot=64, rng=rng)
    idx = rng.integers(0, len(frames), n)
    exp = w.exp.take(idx)
    if ns:
        st = exp.start.astype(np.int64)
        assert st[1] > st[0] == 0 and st[254] > st[253] and st[255] > st[254]
        assert (st[100:111] == st[100]).all() and st[111] > st[110]
    else:
        assert (exp.start[:255] == 0).all() and exp.start[255] == n
    run_demux(buf, offs[idx], lens[idx], w, exp, gpu)


def test_demux_all_unbound(gpu, world):
    rng = np.random.default_rng(6)
    w = World(world.socks, [stray_frame(rng) for _ in range(700)])
    assert (w.exp.sock == model.UNBOUND).all() and w.exp.start[254] == 0
    run_demux(*slot_ring(w.frames, rng=rng), w, w.exp, gpu)


def test_demux_none_delivered(gpu, world):
    """All ARP: every id NONE, all starts 0, the sentinel-filled list untouched."""
    rng = np.random.default_rng(7)
    w = World(world.socks, rx_ring(rng, 300, cases=("arp",)))
    assert (w.exp.sock == model.NONE).all() and not w.exp.start.any()
    run_demux(*slot_ring(w.frames, rng=rng), w, w.exp, gpu)


def test_demux_precedence_and_lookalikes(gpu, world):
    """Connected over bound on one local pair, and the IPv4 / IPv6 sockets
    alike in four address bytes and both ports."""
    rng = np.random.default_rng(8)
    p = be16(4433)
    cases = [((4, A4[0], p, PEER4, be16(999)), 1), ((4, A4[0], p, PEER4, be16(1000)), 4),
             ((4, A4[0], p, PEER4, be16(998)), 0), ((4, A4[0], p, bytes([192, 168, 7, 8]), be16(999)), 0),
             ((6, A6[0], p, PEER6, be16(999)), 3), ((6, A6[0], p, PEER4 + PEER6[4:], be16(999)), 2),
             ((6, A4[0] + bytes(12), p, PEER6, be16(999)), model.UNBOUND),
             ((4, A4[0], be16(4434), PEER4, be16(999)), model.UNBOUND),
             ((4, PEER4, be16(999), A4[0], p), model.UNBOUND)]
    w = World(world.socks, [udp_frame(rng, *c) for c, _ in cases] * 3)
    assert w.exp.sock.tolist() == [want for _, want in cases] * 3
    run_demux(*pack(w.frames, lead=5), w, w.exp, gpu)


# --- call variants ------------------------------------------------------------

def test_demux_ids_only(gpu, world):
    buf, offs, lens = slot_ring(world.frames)
    run_demux(buf, offs, lens, world, world.exp, gpu, want_list=False)


def test_demux_empty(gpu, world):
    z8 = torch.zeros(64, dtype=torch.uint8, device=gpu)
    o = torch.zeros(0, dtype=torch.int64, device=gpu)
    rec = torch.zeros((0, 16), dtype=torch.uint8, device=gpu)
    sock, lst, start = wc.rx_demux(z8, o, rec, dev(world.tab, gpu), world.ns)
    assert sock.numel() == 0 and lst.numel() == 0 and not start.cpu().numpy().any()
    # the empty call writes the starts, it does not leave them
    from warpcore_amd import _lib
    start = torch.full((256,), 7, dtype=torch.int64, device=gpu)
    lst = sentinel_list(1, gpu)
    st = torch.cuda.current_stream(gpu).cuda_stream
    assert _lib.active().wc_rx_demux(None, None, None, 0, None, 0, None, lst.data_ptr(),
                                     start.data_ptr(), None, st) == 0
    assert not start.cpu().numpy().any() and int(lst.cpu().numpy().view(np.uint32)[0]) == SENTINEL
    hv, hrec, hsock, hlst, hstart, hdrops = wc.rx_demux_host(
        np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint16), world.tab, world.ns)
    assert (hv.size, hrec.size, hsock.size, hlst.size, hdrops) == (0, 0, 0, 0, 0)
    assert not hstart.any()


def test_demux_two_streams(gpu, world):
    """Two calls at once on two streams, each with its own scratch and its own
    table: no library state is shared between them."""
    n = 2 * BLOCK + 100
    buf, offs, lens = slot_ring(world.frames, rng=np.random.default_rng(9))
    other = World(population(254, 9)[::-1].copy(), world.frames)
    t = dev(buf, gpu)
    runs = []
    for k, w in enumerate((world, other)):
        idx = (np.arange(n) * (3 + 2 * k)) % len(world.frames)
        o = dev(offs[idx], gpu)
        _, rec, _, _, _ = wc.rx_deliver_ragged(t, o, dev(lens[idx], gpu), want_list=False)
        scratch = torch.empty(wc.rx_demux_scratch(n) // 4, dtype=torch.int32, device=gpu)
        runs.append((w, idx, o, rec, dev(w.tab, gpu), sentinel_list(n, gpu), scratch,
                     torch.cuda.Stream(gpu)))
    torch.cuda.synchronize(gpu)
    outs = []
    for w, idx, o, rec, tab, lst, scratch, st in runs:
        outs.append(wc.rx_demux(t, o, rec, tab, w.ns, out_list=lst, scratch=scratch, stream=st))
    for *_, st in runs:
        st.synchronize()
    for (w, idx, *_), (sock, lst, start) in zip(runs, outs):
        check(sock, lst, start, w.exp.take(idx), n)


def test_demux_70000_frames_twice(gpu, world):
    """Eighteen blocks, run twice into the same buffers: identical output."""
    n = 70000
    buf, offs, lens = slot_ring(world.frames, rng=np.random.default_rng(10))
    idx = (np.arange(n) * 11) % len(world.frames)
    t, o = dev(buf, gpu), dev(offs[idx], gpu)
    _, rec, _, _, _ = wc.rx_deliver_ragged(t, o, dev(lens[idx], gpu), want_list=False)
    tab, lst = dev(world.tab, gpu), sentinel_list(n, gpu)
    scratch = torch.empty(wc.rx_demux_scratch(n) // 4, dtype=torch.int32, device=gpu)
    exp = world.exp.take(idx)
    seen = []
    for _ in range(2):
        sock, got, start = wc.rx_demux(t, o, rec, tab, world.ns, out_list=lst, scratch=scratch)
        check(sock, got, start, exp, n)
        seen.append((sock.cpu().numpy().tobytes(), got.cpu().numpy().tobytes(),
                     start.cpu().numpy().tobytes()))
    assert seen[0] == seen[1]


# --- the host call ------------------------------------------------------------

def check_host(got, w, idx):
    v, rec, sock, lst, start, drops = got
    exp = w.exp.take(idx)
    np.testing.assert_array_equal(v, w.dexp.verdicts[idx])
    assert (rec == w.dexp.records[idx]).all()
    assert drops == int(np.isin(w.dexp.verdicts[idx], wc.RX_DROPS).sum())
    np.testing.assert_array_equal(sock, exp.sock)
    np.testing.assert_array_equal(start, exp.start)
    np.testing.assert_array_equal(lst, exp.list)


@pytest.mark.parametrize("register", [False, True])
@pytest.mark.parametrize("n", [64, 4096, 200000])
def test_demux_host(gpu, world, register, n):
    """The ring in host memory: a zero-copy launch for a small registered
    batch, the in-place stream for a large one, the pipeline for pageable
    memory.  Verdicts, records and drops are wc_rx_deliver_host's for the same
    frames; never the resident server, and nothing falls back."""
    buf, offs, lens = slot_ring(world.frames, rng=np.random.default_rng(n))
    idx = (np.arange(n) * 3) % len(world.frames)
    offs, lens = offs[idx], lens[idx]
    if register:
        wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        got = wc.rx_demux_host(buf, offs, lens, world.tab, world.ns)
        dv, drec, dlst, ddrops = wc.rx_deliver_host(buf, offs, lens)
    finally:
        if register:
            wc.host_unregister(buf)
    s1 = wc.server_stats()
    check_host(got, world, idx)
    np.testing.assert_array_equal(got[0], dv)
    assert (got[1] == drec).all() and got[5] == ddrops
    np.testing.assert_array_equal(np.sort(got[3]), dlst)
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (0, 0)


def test_demux_host_dense_ascending(gpu, world):
    """Registered, dense and ascending, too large for one zero-copy launch:
    the pipeline's range copy straight from the region."""
    reps = 10
    buf, offs, lens = pack(world.frames * reps, align=1, lead=1)
    idx = np.arange(len(world.frames) * reps) % len(world.frames)
    wc.host_register(buf)
    try:
        got = wc.rx_demux_host(buf, offs, lens, world.tab, world.ns)
    finally:
        wc.host_unregister(buf)
    check_host(got, world, idx)


def test_c_rx_demux_loop(gpu, tmp_path):
    """INTEGRATION.md's demux hook compiled in C (tests/c/rx_demux_loop.c): an
    engine-shaped loop -- ring, wc_rx_deliver_host / wc_rx_demux_host,
    per-socket queues -- whose queues equal those of a plain per-frame loop
    doing udp.c:141-156 over the same frames.  A small ring (one zero-copy
    launch) and a large one (in-place stream, pipeline)."""
    from cprog import build
    exe = build("rx_demux_loop", tmp_path)
    for slots in ("1024", "6000"):
        r = subprocess.run([str(exe), slots], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "rx_demux_loop: ok" in r.stdout
