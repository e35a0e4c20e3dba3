"""GPU tests of the RX drain (wc_rx_drain): all fifteen outputs against
tests/rx_drain_cases.expect -- the models alone -- AND against the four-call
chain (rx_deliver_ragged -> rx_demux -> rx_reply_plan -> rx_neigh_plan) run on
the same tensors, bit-exact.  Every output array is pre-filled with 0xA5 and
stands between guard bytes: list entries at and past a count, the guards and
the RX buffer must be untouched; *drops starts at 7 and is added to.

A frame's six per-frame results depend on its bytes and the two tables alone,
not on where the frame lies, so one expectation per base world (600 frames at
most) is computed once and every size is run as n offsets that point at the
same frames; the lists are regrouped from the per-frame expectation."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rx_deliver_model as dmodel
import rx_demux_cases as dc
import rx_demux_model as xmodel
import rx_drain_cases as cases
import rx_neigh_cases as nc
import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel
import warpcore_amd as wc
from warpcore_amd import _lib
from warpcore_amd.cksum import _DrainOut

pytestmark = pytest.mark.gpu

FILL, GUARD, DROPS0 = 0xA5, 64, 7
SMALL = cases.SMALL
SIZES = [1, 63, 64, 65, 129, 600, SMALL - 1, SMALL, SMALL + 1]
PER_FRAME = ("verdicts", "records", "sock", "actions", "reply_lens", "nact")
# list -> (its count: where it is written, the expectation's name)
LISTS = {"list": "start", "reply_list": "reply_count", "neigh_reply_list": "neigh_reply_count",
         "update_list": "update_count"}


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def dev_bytes(a: np.ndarray, d) -> torch.Tensor:
    return dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy(), d)


class Outs:
    """wc_rx_drain's fifteen arrays, each 0xA5-filled between 64 guard bytes."""

    def __init__(self, d, n: int, drops: int = DROPS0):
        nl = max(n, 1)
        spec = {"verdicts": (n, torch.uint8), "records": (16 * n, torch.uint8),
                "drops": (8, torch.int64), "sock": (n, torch.uint8), "list": (4 * nl, torch.int32),
                "start": (8 * 256, torch.int64), "actions": (n, torch.uint8),
                "reply_lens": (2 * n, torch.uint16), "reply_list": (4 * nl, torch.int32),
                "reply_count": (8, torch.int64), "nact": (n, torch.uint8),
                "neigh_reply_list": (4 * nl, torch.int32), "neigh_reply_count": (8, torch.int64),
                "update_list": (4 * nl, torch.int32), "update_count": (8, torch.int64)}
        assert list(spec) == list(wc.RxDrain._fields)
        self.n, self.raw, self.nbytes, views = n, {}, {}, {}
        for name, (nbytes, dtype) in spec.items():
            raw = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device=d)
            self.raw[name], self.nbytes[name] = raw, nbytes
            views[name] = raw[GUARD:GUARD + nbytes].view(dtype)
        views["records"] = views["records"].view(n, 16)
        views["drops"].fill_(drops)
        self.out = wc.RxDrain(**views)

    def fetch(self):
        """Everything to the host; the guards checked."""
        self.host = {k: r.cpu().numpy() for k, r in self.raw.items()}
        for name, h in self.host.items():
            nb = self.nbytes[name]
            assert (h[:GUARD] == FILL).all() and (h[GUARD + nb:] == FILL).all(), f"guard of {name}"
        return self

    def get(self, name: str, dtype=np.uint8) -> np.ndarray:
        return self.host[name][GUARD:GUARD + self.nbytes[name]].view(dtype)

    def count(self, name: str) -> int:
        return int(self.get(name, np.uint64)[255 if name == "start" else 0])


def regroup(per, ns: int):
    """The whole expectation of a batch from its per-frame part."""
    e = SimpleNamespace(**{k: getattr(per, k) for k in PER_FRAME})
    e.n = len(e.verdicts)
    e.drops = int(np.isin(e.verdicts, (2, 3, 4, 5, 6, 9)).sum())
    e.list, e.start = xmodel.group(e.sock, ns)
    e.reply_list = dmodel.select(e.actions, rmodel.MASK_REPLY)
    e.neigh_reply_list = dmodel.select(e.nact, nmodel.MASK_REPLY)
    e.update_list = dmodel.select(e.nact, nmodel.MASK_UPDATE)
    return e


class World:
    """Base frames in a layout, the two tables, and the models' expectation of
    them, computed once; run(): n offsets over those frames through the drain."""

    def __init__(self, d, frames, socks, eng, slot: int, layout: str = "packed", seed: int = 1):
        self.d, self.ns, self.slot, self.eng = d, len(socks), slot, eng
        self.tab = wc.rx_socktab_build(socks)
        self.buf, self.offs, self.lens = cases.layout(layout, frames, seed)
        self.base = cases.expect(self.buf, self.offs, self.lens, self.tab, self.ns, eng, slot)
        self.d_buf, self.d_tab, self.d_eng = dev(self.buf, d), dev_bytes(self.tab, d), dev_bytes(eng, d)

    def index(self, n: int) -> np.ndarray:
        m = len(self.offs)
        step = next(p for p in (7, 11, 13, 17, 19) if m % p)  # coprime: every frame is reached
        return np.arange(n) if n == m else (np.arange(n) * step + n) % m

    def expect(self, n: int):
        idx = self.index(n)
        per = SimpleNamespace(**{k: getattr(self.base, k)[idx] for k in PER_FRAME})
        per.records = per.records.view(np.uint8).reshape(n, 16)
        return regroup(per, self.ns)

    def inputs(self, n: int):
        idx = self.index(n)
        return dev(self.offs[idx], self.d), dev(self.lens[idx], self.d)

    def run(self, n: int, stream=None, outs=None, scratch=None, d_off=None, d_len=None):
        if d_off is None:
            d_off, d_len = self.inputs(n)
        outs = Outs(self.d, n) if outs is None else outs
        wc.rx_drain(self.d_buf, d_off, d_len, self.d_tab, self.ns, self.d_eng, self.slot,
                    out=outs.out, scratch=scratch, stream=stream)
        return outs

    def chain(self, n: int):
        """The four calls on the same tensors, every result on the host."""
        d_off, d_len = self.inputs(n)
        v, rec, _, _, drops = wc.rx_deliver_ragged(self.d_buf, d_off, d_len, want_list=False)
        sock, lst, start = wc.rx_demux(self.d_buf, d_off, rec, self.d_tab, self.ns)
        act, rlen, rl, rcnt = wc.rx_reply_plan(self.d_buf, d_off, d_len, v, sock, self.d_eng, self.slot)
        nact, nrl, nrcnt, ul, ucnt = wc.rx_neigh_plan(self.d_buf, d_off, d_len, act, self.d_eng)
        torch.cuda.synchronize()
        h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)  # noqa: E731
        c = SimpleNamespace(verdicts=h(v), records=h(rec).reshape(n, 16), sock=h(sock), actions=h(act),
                            reply_lens=h(rlen, np.uint16), nact=h(nact), start=h(start, np.uint64),
                            drops=int(drops.item()), n=n)
        for name, lt, cnt in (("list", lst, int(c.start[255])), ("reply_list", rl, int(rcnt.item())),
                              ("neigh_reply_list", nrl, int(nrcnt.item())),
                              ("update_list", ul, int(ucnt.item()))):
            setattr(c, name, h(lt, np.uint32)[:cnt])
        return c


def check(o: Outs, e, what: str):
    """The drain's fetched outputs against an expectation (models or chain)."""
    n = e.n
    for name, dt in (("verdicts", np.uint8), ("sock", np.uint8), ("actions", np.uint8),
                     ("nact", np.uint8), ("reply_lens", np.uint16)):
        got, want = o.get(name, dt), getattr(e, name)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, bad[:8], got[bad[:8]], want[bad[:8]])
    bad = np.flatnonzero((o.get("records").reshape(n, 16) != e.records).any(axis=1))
    assert bad.size == 0, (what, "records", bad[:8])
    assert int(o.get("drops", np.uint64)[0]) == DROPS0 + e.drops, (what, "drops")
    np.testing.assert_array_equal(o.get("start", np.uint64), e.start, err_msg=what)
    for name, cname in LISTS.items():
        want, got = getattr(e, name), o.get(name, np.uint32)
        assert o.count(cname) == len(want), (what, cname, o.count(cname), len(want))
        np.testing.assert_array_equal(got[:len(want)], want, err_msg=f"{what} {name}")
        assert (got[len(want):] == 0xA5A5A5A5).all(), (what, name, "written past its count")


def run_both_ways(w: World, n: int):
    o = w.run(n)
    torch.cuda.synchronize()
    o.fetch()
    check(o, w.expect(n), "models")
    check(o, w.chain(n), "chain")
    assert (w.d_buf.cpu().numpy() == w.buf).all(), "the RX buffer was written"
    return o


@pytest.fixture(scope="module")
def worlds(gpu):
    out = {}
    for name, (seed, n, ns, slot) in cases.WORLDS.items():
        frames, socks = cases.world(seed, n, ns)
        out[name] = World(gpu, frames, socks, rc.engine_table(rng=np.random.default_rng(seed)), slot,
                          name, seed)
    return out


@pytest.mark.parametrize("layout", list(cases.WORLDS))
@pytest.mark.parametrize("n", SIZES)
def test_both_ways_of_knowing_the_answer(worlds, n, layout):
    """n = 4097: the fallback; 4095 / 4096: the list workgroup's last partial
    and last full wave step."""
    o = run_both_ways(worlds[layout], n)
    if n >= 600:  # a world that exercises every list
        assert min(o.count(c) for c in LISTS.values()) > 0


def test_determinism_and_drops(worlds):
    w = worlds["packed"]
    for n in (600, SMALL):
        a, b = w.run(n), w.run(n)
        torch.cuda.synchronize()
        a.fetch(), b.fetch()
        for name in a.host:
            assert (a.host[name] == b.host[name]).all(), name
        e = w.expect(n)
        assert e.drops > 0 and int(a.get("drops", np.uint64)[0]) == DROPS0 + e.drops
    # accumulated: a second call on the same outputs adds the count again
    a = w.run(600)
    w.run(600, outs=a)
    torch.cuda.synchronize()
    assert int(a.fetch().get("drops", np.uint64)[0]) == DROPS0 + 2 * w.expect(600).drops


def tiled(gpu, frames, socks, eng=None, slot=256):
    eng = rc.engine_table() if eng is None else eng
    return World(gpu, frames, socks, eng, slot, "packed", len(frames) % 16)


def test_extreme_every_frame_to_one_socket(gpu):
    rng = np.random.default_rng(31)
    socks = cases.sockets(6, 31)
    w = tiled(gpu, [dc.frame_to(rng, socks[2])[0] for _ in range(64)], socks)
    o = run_both_ways(w, SMALL)
    start = o.get("start", np.uint64)
    assert (o.get("sock") == 2).all() and start[2] == 0 and (start[3:] == SMALL).all()
    assert (o.get("list", np.uint32) == np.arange(SMALL)).all()


def test_extreme_every_frame_unbound(gpu):
    rng = np.random.default_rng(32)
    w = tiled(gpu, [dc.stray_frame(rng)[0] for _ in range(64)], cases.sockets(6, 32))
    o = run_both_ways(w, SMALL)
    start = o.get("start", np.uint64)
    assert (o.get("sock") == xmodel.UNBOUND).all() and (start[:255] == 0).all() and start[255] == SMALL


def test_extreme_no_frame_delivered_all_arp(gpu):
    frames = [f[0] for f in nc.world(33, 66) if f[0][12:14] == b"\x08\x06"]
    assert len(frames) >= 20
    w = tiled(gpu, frames, cases.sockets(6, 33))
    o = run_both_ways(w, SMALL)
    assert (o.get("sock") == xmodel.NONE).all() and not o.get("start", np.uint64).any()
    assert (o.get("list", np.uint32) == 0xA5A5A5A5).all() and not o.get("records").any()
    assert o.count("update_count") > o.count("neigh_reply_count") > 0 and o.count("reply_count") == 0


@pytest.mark.parametrize("ns", [0, 1, 254])
def test_extreme_socket_counts(gpu, ns):
    rng = np.random.default_rng(40 + ns)
    socks = cases.sockets(ns, 40 + ns)
    frames = [dc.frame_to(rng, s, max_payload=40)[0] for s in socks]
    frames += [dc.stray_frame(rng, max_payload=40)[0] for _ in range(10)]
    frames += [f[0] for f in rc.world(40 + ns, 30)]
    frames = [frames[i] for i in rng.permutation(len(frames))]
    w = tiled(gpu, frames, socks)
    o = run_both_ways(w, SMALL)
    hit = set(o.get("sock").tolist()) - {xmodel.NONE, xmodel.UNBOUND}
    assert hit == set(range(ns)) and (ns < 254 or len(hit) >= 200)


def test_engine_table_without_an_ipv4_address(gpu, worlds):
    src = worlds["slots"]
    seed, n, ns, slot = cases.WORLDS["slots"]
    frames, socks = cases.world(seed, n, ns)
    w = World(gpu, frames, socks, rc.engine_table(v4=0), slot, "slots", seed)
    o = run_both_ways(w, SMALL)
    arp = np.array([fr[12:14] == b"\x08\x06" for fr in w.base.frames])[w.index(SMALL)]
    assert arp.sum() > 100 and not o.get("nact")[arp].any()  # eth.c:80: no ARP without an address
    assert (o.get("actions") != src.expect(SMALL).actions).any()


def test_empty_batch(gpu, worlds):
    w = worlds["slots"]
    o = w.run(0)
    torch.cuda.synchronize()
    o.fetch()
    assert not o.get("start", np.uint64).any()
    assert [o.count(c) for c in LISTS.values()] == [0, 0, 0, 0]
    assert int(o.get("drops", np.uint64)[0]) == DROPS0
    for name in LISTS:
        assert (o.get(name, np.uint32) == 0xA5A5A5A5).all()
    # NULL everywhere else: the four counts and start alone
    o = Outs(gpu, 0)
    members = dict(start=o.out.start, rcount=o.out.reply_count, nrcount=o.out.neigh_reply_count,
                   ucount=o.out.update_count)
    c_out = _DrainOut(**{k: t.data_ptr() for k, t in members.items()})
    rc_ = _lib.active().wc_rx_drain(None, None, None, 0, None, 0, None, 0, ctypes.byref(c_out), None,
                                    torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    o.fetch()
    assert rc_ == 0 and not o.get("start", np.uint64).any()
    assert [o.count(c) for c in LISTS.values()] == [0, 0, 0, 0]


def test_two_streams(gpu, worlds):
    """Two streams with their own scratch and outputs in one process, 20 calls
    each on different worlds and sizes."""
    plan = [(worlds["slots"], 600, torch.cuda.Stream(gpu)), (worlds["packed"], SMALL, torch.cuda.Stream(gpu))]
    state = []
    for w, n, st in plan:
        d_off, d_len = w.inputs(n)
        scratch = torch.empty(max(1, wc.rx_drain_scratch(n) // 4 + 1), dtype=torch.int32, device=gpu)
        state.append((w, n, st, d_off, d_len, scratch, [Outs(gpu, n) for _ in range(20)]))
    torch.cuda.synchronize()
    for k in range(20):
        for w, n, st, d_off, d_len, scratch, outs in state:
            w.run(n, stream=st, outs=outs[k], scratch=scratch, d_off=d_off, d_len=d_len)
    torch.cuda.synchronize()
    for w, n, st, d_off, d_len, scratch, outs in state:
        e = w.expect(n)
        for o in outs:
            check(o.fetch(), e, f"stream of n = {n}")


def test_hand_over_to_the_builders(gpu, worlds):
    """The drain's lists and counts go into the existing build calls; the built
    frames and records are the models'."""
    w = worlds["slots"]
    n = len(w.offs)
    d_off, d_len = w.inputs(n)
    o = w.run(n, d_off=d_off, d_len=d_len)
    r, ex = o.out, w.base
    rng = np.random.default_rng(5)
    m_r, m_n, m_u = len(ex.reply_list) + 5, len(ex.neigh_reply_list) + 5, len(ex.update_list) + 5
    out0, out_offs = rc.out_slots(m_r, w.slot, rng)
    d_out = dev(out0, gpu)
    olen, built = wc.rx_reply_build(w.d_buf, d_off, d_len, r.actions, r.reply_list, r.reply_count,
                                    w.d_eng, d_out, dev(out_offs, gpu), w.slot)
    nout0, nout_offs = rc.out_slots(m_n, w.slot, rng)
    d_nout = dev(nout0, gpu)
    nolen, nbuilt = wc.rx_neigh_build(w.d_buf, d_off, d_len, r.nact, r.neigh_reply_list,
                                      r.neigh_reply_count, w.d_eng, d_nout, dev(nout_offs, gpu), w.slot)
    upd = wc.rx_neigh_updates(w.d_buf, d_off, d_len, r.nact, r.update_list, r.update_count, m_u)
    torch.cuda.synchronize()
    check(o.fetch(), w.expect(n), "models")
    want, want_len, want_built = ex.reply.built(out0, out_offs)
    assert (olen.cpu().numpy() == want_len).all() and int(built.item()) == want_built > 0
    assert (d_out.cpu().numpy() == want).all()
    want, want_len, want_built = ex.neigh.built(nout0, nout_offs, w.slot)
    assert (nolen.cpu().numpy() == want_len).all() and int(nbuilt.item()) == want_built > 0
    assert (d_nout.cpu().numpy() == want).all()
    want = ex.neigh.updates(m_u)
    assert want.any() and (upd.cpu().numpy().reshape(m_u, 24) == want).all()
