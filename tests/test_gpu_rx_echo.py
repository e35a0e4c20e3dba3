"""GPU tests of the RX echo (wc_rx_echo): every output against
tests/rx_echo_model.py in both modes, the copy at every source and destination
phase, every branch, the maps, and the closed loop drain -> echo -> pump.  The
plan in front is the real wc_rx_drain.  Every output is pre-filled with 0xA5
between 64 guard bytes, the slots lie in random-filled buffers that are compared
whole, *skipped starts at 7, and the RX buffer is compared whole afterwards.

A frame's record depends on its bytes alone, so one expectation per base world
is computed once and every size is run as n offsets that point at the same
frames (test_gpu_rx_drain.World)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rx_deliver_model as dmodel
import rx_demux_cases as dc
import rx_echo_cases as cases
import rx_echo_model as model
import rx_reply_cases as rc
import tx_build_model as bmodel
import tx_neigh_model as tmodel
import warpcore_amd as wc
from test_gpu_rx_answer import Guarded
from test_gpu_rx_drain import World, dev, dev_bytes
from test_rx_echo_model import swapped

pytestmark = pytest.mark.gpu

SKIPPED0, SLOT = 7, 2048
FIELDS = {"descs": 8, "dsts": 24, "af": 1, "status": 1, "src": 4, "tx_off": 8}


@pytest.fixture(scope="module")
def gpu():
    d = torch.device("cuda:0")
    wc.gpu_init(0)
    return d


@pytest.fixture(scope="module")
def world(gpu):
    socks, frames = cases.world(31, 600, 17)
    return World(gpu, frames, socks, rc.engine_table(), 256, "packed", 3)


def slots_of(m: int, slot: int, seed: int = 3):
    """m slots of `slot` bytes in a random-filled buffer, slot j at phase j mod 16."""
    return rc.out_slots(max(m, 1), slot, np.random.default_rng(seed))


class Call:
    """One wc_rx_echo call: guarded outputs, the slots, and the model's
    expectation of both."""

    def __init__(self, w: World, n: int, plan, d_off, d_len, emap, m, copy, ids=True, src=True,
                 slot=SLOT, rec=None, lst=None, want=None, toff=None):
        d = w.d
        self.w, self.n, self.m, self.copy, self.slot = w, n, m, copy, slot
        self.d_off, self.d_len, self.plan = d_off, d_len, plan
        self.emap = np.asarray(emap, np.uint16)
        self.d_map = dev(self.emap.view(np.int16), d)
        self.ids = np.random.default_rng(m).integers(0, 1 << 16, max(m, 1)).astype(np.uint16) \
            if ids else None
        self.d_ids = dev(self.ids.view(np.int16), d) if ids else None
        self.g = {k: Guarded(d, size * m) for k, size in FIELDS.items()}
        self.count, self.skipped = Guarded(d, 8, torch.int64), Guarded(d, 8, torch.int64)
        self.skipped.view.fill_(SKIPPED0)
        self.rec = plan.records if rec is None else rec
        self.lst = plan.list if lst is None else lst
        self.with_src = src
        if copy:
            self.tbuf, self.toff = slots_of(m, slot)
            if toff is not None:
                self.toff = toff
            self.d_tbuf, self.d_toff = dev(self.tbuf.copy(), d), dev(self.toff[:m], d)
        self.want = want

    def run(self, stream=None, check=True):
        g = self.g
        out = wc.RxEcho(g["descs"].view, g["dsts"].view, g["af"].view, g["status"].view,
                        g["src"].view.view(torch.int32) if self.with_src else None,
                        None if self.copy else g["tx_off"].view.view(torch.int64),
                        self.count.view, self.skipped.view)
        kw = dict(out_base=self.d_tbuf, out_offsets=self.d_toff) if self.copy else dict(m=self.m)
        self.out = wc.rx_echo(self.w.d_buf, self.d_off, self.d_len,
                              (self.rec, self.lst, self.plan.start), self.d_map,
                              out_slot_bytes=self.slot, ip_ids=self.d_ids, out=out, stream=stream,
                              check=check, **kw)
        return self

    def fetch(self) -> dict:
        torch.cuda.synchronize()
        got = {k: g.get() for k, g in self.g.items()}
        got["count"] = int(self.count.get(np.uint64)[0])
        got["skipped"] = int(self.skipped.get(np.uint64)[0])
        got["slots"] = self.d_tbuf.cpu().numpy() if self.copy else None
        got["rx"] = self.w.d_buf.cpu().numpy()
        return got

    def expect(self, e) -> dict:
        """The model's outputs as the bytes the call must leave."""
        m = self.m
        want = {"descs": e.desc.tobytes(), "dsts": e.dsts.tobytes(), "af": e.af.tobytes(),
                "status": e.status.tobytes(),
                "src": e.src.tobytes() if self.with_src else b"\xa5" * (4 * m),
                "tx_off": b"\xa5" * (8 * m) if self.copy else e.tx_off.tobytes(),
                "count": e.E, "skipped": SKIPPED0 + e.skipped, "slots": None, "rx": self.w.buf}
        if self.copy:
            t = self.tbuf.copy()
            for j in range(m):
                if e.payload[j] is not None:
                    at = int(self.toff[j]) + bmodel.hdr_len(int(e.af[j]))
                    t[at:at + len(e.payload[j])] = np.frombuffer(e.payload[j], np.uint8)
            want["slots"] = t
        return want


def same(got: dict, want: dict, what: str):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, bytes):
            g = g.tobytes()
        if isinstance(w, np.ndarray):
            assert np.array_equal(g, w), f"{what}: {k}"
        else:
            assert g == w, f"{what}: {k}"


def modelled(w: World, n: int, emap, m, copy, slot=SLOT, ids=None, rec=None, lst=None):
    e = w.expect(n)
    idx = w.index(n)
    return model.echo(w.buf, w.offs[idx], w.lens[idx], e.records.copy() if rec is None else rec,
                      e.list if lst is None else lst, e.start, emap, m, copy, slot, ids, n=n)


def drained(w: World, n: int):
    d_off, d_len = w.inputs(n)
    return w.run(n, d_off=d_off, d_len=d_len).out, d_off, d_len


KIND = {1: "all", 63: "alternating", 64: "all", 65: "alternating", 600: "alternating", 4096: "all"}


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "in_place"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 600, 4096])
def test_parity_with_the_model(world, n, copy):
    w = world
    plan, d_off, d_len = drained(w, n)
    emap = cases.echo_map(w.ns, KIND[n])
    E = modelled(w, n, emap, 0, copy).E
    assert E > 0 or n == 1
    runs = [(max(E - 1, 0), True, True), (E, True, True), (E, False, True), (E, True, False),
            (E, False, False), (E + 5, False, True)]
    for m, ids, src in runs:
        c = Call(w, n, plan, d_off, d_len, emap, m, copy, ids, src).run()
        e = modelled(w, n, emap, m, copy, ids=c.ids)
        assert e.E == E and e.skipped == 0
        same(c.fetch(), c.expect(e), f"n {n}, m {m}, ids {ids}, src {src}")


def test_copy_at_every_source_and_destination_phase(gpu):
    """256 frames to one bound socket in a packed ring: the payload of frame j
    starts at source phase (c + j) mod 16; slot j is laid so that its payload
    starts at destination phase (j div 16) mod 16."""
    rng = np.random.default_rng(12)
    socks = dc.population(1, 1)
    frames = [cases.sized_frame_to(rng, socks[0], cases.LENS[(j + j // 16) % len(cases.LENS)], j)[0]
              for j in range(256)]
    w = World(gpu, frames, socks, rc.engine_table(), 256, "packed", 5)
    plan, d_off, d_len = drained(w, 256)
    emap = cases.echo_map(1, "all")
    toff, pos = [], 64
    for j in range(256):
        pos += (j // 16 - (pos + 42)) % 16
        toff.append(pos)
        pos += SLOT + 5
    tbuf = np.random.default_rng(4).integers(0, 256, pos + 64, dtype=np.uint8)
    c = Call(w, 256, plan, d_off, d_len, emap, 256, True, toff=np.array(toff, np.uint64))
    c.tbuf, c.d_tbuf = tbuf, dev(tbuf.copy(), gpu)
    c.run()
    e = modelled(w, 256, emap, 256, True, ids=c.ids)
    assert e.E == 256 and (e.status == model.ECHO).all()
    sp = [(w.d_buf.data_ptr() + int(w.offs[int(e.src[j])]) + 42) % 16 for j in range(256)]
    dp = [(c.d_tbuf.data_ptr() + toff[j] + 42) % 16 for j in range(256)]
    assert len(set(zip(sp, dp))) == 256, "every phase pair"
    assert set(cases.LENS) == set(e.desc["data_len"].tolist())
    same(c.fetch(), c.expect(e), "phases")


def test_every_branch(world, gpu):
    w, n = world, 600
    plan, d_off, d_len = drained(w, n)
    emap = cases.echo_map(w.ns, "all")
    base = modelled(w, n, emap, 0, True)
    E, m = base.E, base.E + 3
    base = modelled(w, n, emap, m, True)
    idx = w.index(n)
    lens = w.lens[idx]
    ex = w.expect(n)
    rec = ex.records.copy().view(dmodel.RECORD).reshape(-1)
    lst = np.zeros(n, np.uint32)            # n entries, as the drain's list has
    lst[:len(ex.list)] = ex.list
    i0, i1, i2 = (int(base.src[j]) for j in (0, 1, 2))
    rec[i0]["data_len"] = int(lens[i0]) - int(rec[i0]["data_off"]) + 1   # one byte past the frame
    rec[i1]["data_len"] = int(lens[i1]) - int(rec[i1]["data_off"])       # the exact fit
    rec[i2]["af"] = 5
    pos3 = int(np.flatnonzero(ex.list == base.src[3])[0])
    lst[pos3] = n                                                        # names no frame
    # records no delivery writes, one rule of STALE each: a header shorter than the built one
    # (data_off kept consistent with it), a data_off off 14 + hl + 8, a source address that
    # ends one byte past the frame
    i4, i5, i6 = (int(base.src[j]) for j in (4, 5, 6))
    rec[i4]["hl"], rec[i4]["data_off"] = 16, 14 + 16 + 8
    rec[i5]["data_off"] = int(rec[i5]["data_off"]) - 1
    rec[i6]["src_off"] = int(lens[i6]) - (4 if int(rec[i6]["af"]) == 4 else 16) + 1
    d_rec, d_lst = dev_bytes(rec, gpu).reshape(n, 16), dev(lst.view(np.int32), gpu).view(torch.uint32)
    for copy in (True, False):
        c = Call(w, n, plan, d_off, d_len, emap, m, copy, rec=d_rec, lst=d_lst).run()
        e = modelled(w, n, emap, m, copy, ids=c.ids, rec=rec, lst=lst)
        assert e.status[:7].tolist() == [model.SHORT, model.ECHO] + [model.STALE] * 5
        assert e.skipped == 6 and e.E == E
        for j in (0, 2, 3, 4, 5, 6):        # inert: nothing of the frame in the entry
            assert e.payload[j] is None and e.af[j] == 0 and not e.dsts[j].tobytes().strip(b"\0")
            assert e.desc[j].tolist() == (0xFFFF, 0, 0, 0, j) and e.tx_off[j] == 0
        same(c.fetch(), c.expect(e), f"forged, copy {copy}")
    # out_slot_bytes at the exact fit of a 200-byte IPv4 payload and one below it
    j4 = int(np.flatnonzero((base.desc["data_len"][:E] == 200) & (base.af[:E] == 4))[0])
    for slot, st in ((242, model.ECHO), (241, model.NO_ROOM)):
        c = Call(w, n, plan, d_off, d_len, emap, m, True, slot=slot).run()
        e = modelled(w, n, emap, m, True, slot=slot, ids=c.ids)
        assert e.status[j4] == st and (e.status[:E] == model.NO_ROOM).sum() == e.skipped > 0
        assert (e.status[:E] == model.ECHO).any()
        same(c.fetch(), c.expect(e), f"slot {slot}")
        c = Call(w, n, plan, d_off, d_len, emap, m, False, slot=slot).run()   # no slot, no bound
        e = modelled(w, n, emap, m, False, slot=slot, ids=c.ids)
        assert e.skipped == 0
        same(c.fetch(), c.expect(e), f"in place, slot {slot}")


def test_maps(world, gpu):
    w, n = world, 600
    plan, d_off, d_len = drained(w, n)
    for copy in (True, False):
        # all off: E = 0 and m inert entries
        emap = cases.echo_map(w.ns, "none")
        c = Call(w, n, plan, d_off, d_len, emap, 70, copy).run()
        e = modelled(w, n, emap, 70, copy, ids=c.ids)
        assert e.E == 0 and (e.status == model.NONE).all()
        same(c.fetch(), c.expect(e), "all off")
        # a map value of 256 is off like any other above 255
        emap = cases.echo_map(w.ns, "all")
        emap[0], emap[2] = 256, 0x8000
        c = Call(w, n, plan, d_off, d_len, emap, 400, copy).run()
        e = modelled(w, n, emap, 400, copy, ids=c.ids)
        assert 0 < e.E < modelled(w, n, cases.echo_map(w.ns, "all"), 0, copy).E
        assert 0 not in e.sock[:e.E] and 2 not in e.sock[:e.E]
        same(c.fetch(), c.expect(e), "256 is off")
        # ns = 0: no socket, no RX pointer
        c = Call(w, n, plan, d_off, d_len, np.zeros(0, np.uint16), 5, copy).run()
        e = modelled(w, n, np.zeros(0, np.uint16), 5, copy, ids=c.ids)
        assert e.E == 0
        same(c.fetch(), c.expect(e), "ns = 0")
    # n = 0 with m = 5: no frame, no RX pointer
    plan0 = SimpleNamespace(records=torch.empty((0, 16), dtype=torch.uint8, device=gpu),
                            list=torch.zeros(1, dtype=torch.uint32, device=gpu),
                            start=torch.zeros(256, dtype=torch.int64, device=gpu))
    d_off0, d_len0 = dev(np.zeros(0, np.uint64), gpu), dev(np.zeros(0, np.uint16), gpu)
    for copy in (True, False):
        c = Call(w, 0, plan0, d_off0, d_len0, cases.echo_map(w.ns, "all"), 5, copy).run()
        e = model.echo(w.buf, np.zeros(0, np.uint64), np.zeros(0, np.uint16),
                       np.zeros(0, dmodel.RECORD), np.zeros(0, np.uint32), np.zeros(256, np.uint64),
                       cases.echo_map(w.ns, "all"), 5, copy, SLOT, c.ids, n=0)
        assert e.E == 0 and (e.status == model.NONE).all()
        same(c.fetch(), c.expect(e), "n = 0")
        # m = 0: the count alone
        c = Call(w, n, plan, d_off, d_len, cases.echo_map(w.ns, "all"), 0, copy, ids=False).run()
        e = modelled(w, n, cases.echo_map(w.ns, "all"), 0, copy)
        assert e.E > 0
        same(c.fetch(), c.expect(e), "m = 0")


def test_a_single_socket_on_among_254(gpu):
    socks, frames = cases.world(7, 520, 254)
    w = World(gpu, frames, socks, rc.engine_table(), 256, "packed", 9)
    plan, d_off, d_len = drained(w, 520)
    for one in (0, 130, 253):
        emap = cases.echo_map(254, "single", one=one)
        for copy in (True, False):
            c = Call(w, 520, plan, d_off, d_len, emap, 8, copy).run()
            e = modelled(w, 520, emap, 8, copy, ids=c.ids)
            assert 0 < e.E < 8 and set(e.sock[:e.E]) == {one}
            assert (e.desc["sock"][:e.E] == (one & 0xFF)).all()
            same(c.fetch(), c.expect(e), f"socket {one}")


def test_determinism(world):
    w, n = world, 600
    plan, d_off, d_len = drained(w, n)
    emap = cases.echo_map(w.ns, "alternating")
    for copy in (True, False):
        a = Call(w, n, plan, d_off, d_len, emap, 300, copy).run().fetch()
        b = Call(w, n, plan, d_off, d_len, emap, 300, copy).run().fetch()
        same(a, b, "second run")


def test_two_streams(world, gpu):
    """Two streams with their own outputs, 20 calls each, one in each mode."""
    w = world
    state = []
    for n, copy in ((600, True), (4096, False)):
        plan, d_off, d_len = drained(w, n)
        emap = cases.echo_map(w.ns, "all")
        E = modelled(w, n, emap, 0, copy).E
        calls = [Call(w, n, plan, d_off, d_len, emap, E + 2, copy) for _ in range(20)]
        state.append((calls, torch.cuda.Stream(gpu), modelled(w, n, emap, E + 2, copy,
                                                              ids=calls[0].ids)))
    torch.cuda.synchronize()
    for k in range(20):
        for calls, st, _ in state:
            calls[k].run(stream=st)
    torch.cuda.synchronize()
    for calls, st, e in state:
        for c in calls:
            same(c.fetch(), c.expect(e), "stream")


PEER_MACS = {a: bytes((2, 9, 9, 9, 9, k)) for k, a in enumerate(cases.PEERS4[:2] + cases.PEERS6)}


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "in_place"])
def test_closed_loop_drain_echo_pump(gpu, copy):
    """A ring of datagrams from five peers whose MACs the neighbour table holds
    and one peer (PEERS4[2]) nobody answered for, to bound sockets of both
    families: drain -> echo -> pump on one stream with no host read in between;
    then the built frames go through the RX verdict and delivery."""
    rng = np.random.default_rng(21)
    socks = dc.population(12, 1)
    bound = [s for s in socks if not int(s["connected"])]
    frames = []
    for k in range(90):
        if k % 10 == 9:
            frames.append(dc.stray_frame(rng)[0])
            continue
        s = bound[k % len(bound)]
        ihl = 5 + k % 11 if int(s["af"]) == 4 and k % 4 == 1 else 5
        frames.append(cases.sized_frame_to(rng, s, cases.LENS[k % len(cases.LENS)], k, ihl=ihl)[0])
    w = World(gpu, frames, socks, rc.engine_table(), 256, "slots", 6)
    n = len(frames)
    emap = cases.echo_map(len(socks), "all")
    E = modelled(w, n, emap, 0, copy).E
    m = E + 4
    d_off, d_len = w.inputs(n)
    d_socks = dev_bytes(cases.tx_socks(socks), gpu)
    tab = wc.neigh_tab_init(64, gpu)
    upd = tmodel.records([(4 if len(a) == 4 else 6, mac, a) for a, mac in PEER_MACS.items()])
    wc.neigh_apply(tab, dev_bytes(upd, gpu).reshape(-1, 24),
                   torch.tensor([len(upd)], dtype=torch.int64, device=gpu))
    sol0, sol_off = rc.out_slots(m, 128, rng)
    d_sol, d_sol_off = dev(sol0.copy(), gpu), dev(sol_off, gpu)
    st = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        plan = w.run(n, stream=st, d_off=d_off, d_len=d_len).out
        # behind the drain's launch nothing is read back: the Call's uploads go to the
        # device, and check=False keeps the wrappers from reducing offsets on the host
        c = Call(w, n, plan, d_off, d_len, emap, m, copy).run(stream=st, check=False)
        o = c.out
        if copy:
            p = wc.tx_pump(tab, o.dsts, o.af, o.descs, d_socks, c.d_tbuf, c.d_toff, SLOT, w.d_eng,
                           d_sol, d_sol_off, 128, stream=st, check=False)
        else:  # the RX slots are 2048 bytes; the built frame starts up to 40 bytes in
            p = wc.tx_pump(tab, o.dsts, o.af, o.descs, d_socks, w.d_buf, o.tx_off, 2048 - 40,
                           w.d_eng, d_sol, d_sol_off, 128, stream=st, check=False)
    torch.cuda.synchronize()
    e = modelled(w, n, emap, m, copy, ids=c.ids)
    assert e.E == E and (e.status[:E] == model.ECHO).all()
    got = c.fetch()
    status, flen = p.status.cpu().numpy(), p.frame_lens.cpu().numpy()
    tx = got["slots"] if copy else got["rx"]
    toff = c.toff if copy else e.tx_off
    # the dmac bytes are the pump's to overwrite; everything else is the model's
    dsts = got["dsts"].view(bmodel.DST)
    assert (dsts["addr"] == e.dsts["addr"]).all() and (dsts["port"] == e.dsts["port"]).all()
    same({k: got[k] for k in ("descs", "af", "status", "count")},
         {k: v for k, v in c.expect(e).items() if k in ("descs", "af", "status", "count")}, "echo")
    held = [j for j in range(E) if bytes(e.dsts[j]["addr"][:4]) == cases.PEERS4[2] and e.af[j] == 4]
    built = [j for j in range(E) if j not in held]
    assert held and len(built) > 40
    assert (status[held] == wc.TX_PUMP_HELD).all() and (flen[held] == 0).all()
    assert (status[E:] == wc.TX_MALFORMED).all() and (flen[E:] == 0).all()
    assert int(p.errors.item()) == m - E
    assert (status[built] == wc.TX_SEALED).all()
    # the built frames through the RX verdict and delivery
    b_off = dev(np.asarray(toff, np.uint64)[built], gpu)
    b_len = dev(flen[built], gpu)
    d_tx = c.d_tbuf if copy else w.d_buf
    v0, drops0 = wc.rx_verdict_ragged(d_tx, b_off, b_len)
    v, rec, _, _, drops = wc.rx_deliver_ragged(d_tx, b_off, b_len, want_list=False)
    assert (v.cpu().numpy() == wc.RX_OK).all() and int(drops.item()) == 0
    assert (v0.cpu().numpy() == wc.RX_OK).all() and int(drops0.item()) == 0
    rec = rec.cpu().numpy().view(dmodel.RECORD).reshape(-1)
    idx = w.index(n)
    touched = np.zeros(len(tx), bool)
    for k, j in enumerate(built):
        i = int(e.src[j])
        ro = int(w.offs[idx[i]])
        request = w.buf[ro:ro + int(w.lens[idx[i]])].tobytes()
        rq = dmodel.record_of(request, len(request))
        o_, ln = int(toff[j]), int(flen[j])
        frame = tx[o_:o_ + ln].tobytes()
        assert dmodel.record_of(frame, ln).tobytes() == rec[k].tobytes()
        peer = bytes(e.dsts[j]["addr"][:4 if e.af[j] == 4 else 16])
        assert frame[:6] == PEER_MACS[peer] != request[6:12], "the cached MAC, not the placeholder"
        swapped(request, rq, request[6:12] + frame[6:])
        if not copy:
            assert o_ == ro + int(rq["hl"]) - model.hl_tx(int(e.af[j]))
        touched[o_:o_ + (ln if not copy else bmodel.hdr_len(int(e.af[j])))] = True
    before = c.expect(e)["slots"] if copy else w.buf
    assert np.array_equal(tx[~touched], before[~touched]), "nothing outside the built frames changed"
