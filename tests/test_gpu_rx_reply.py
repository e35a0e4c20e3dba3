"""GPU tests of the RX replies (wc_rx_reply_plan, wc_rx_reply_build) against
tests/rx_reply_model.py, through the real rx_deliver_ragged -> rx_demux ->
rx_reply_plan -> rx_reply_build: actions, reply lengths, list and count, out
lengths, built count, the whole output buffer (random fill, gaps and guard
bytes included) and the whole RX buffer, all exact."""
import numpy as np
import pytest
import torch

import rx_demux_cases
import rx_demux_model
import rx_reply_cases as cases
import rx_reply_model as model
import warpcore_amd as wc

pytestmark = pytest.mark.gpu

ECHO_LENS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
             1472)


def dev_bytes(a: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


@pytest.fixture(scope="module")
def socktab():
    be16 = rx_demux_cases.be16
    socks = np.array([rx_demux_model.sock(4, cases.A4[0], be16(cases.PORT)),
                      rx_demux_model.sock(6, cases.A6[0], be16(cases.PORT))],
                     dtype=rx_demux_model.SOCK)
    return wc.rx_socktab_build(socks), 2


class Run:
    """One batch through the four calls; every result on the host."""

    def __init__(self, dev, socktab, buf, offs, lens, eng, slot, m=None, with_sock=True,
                 ip_ids=False, seed=0, action=None, lst=None):
        rng = np.random.default_rng(1000 + seed)
        self.buf, self.offs, self.lens, self.eng, self.slot = buf, offs, lens, eng, slot
        n = len(offs)
        d_buf = torch.from_numpy(buf.copy()).to(dev)
        d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
        d_eng = dev_bytes(eng, dev)
        v, rec, _, _, _ = wc.rx_deliver_ragged(d_buf, d_off, d_len, want_list=False)
        sock = None
        if with_sock:
            tab, ns = socktab
            sock, _, _ = wc.rx_demux(d_buf, d_off, rec, torch.from_numpy(tab).to(dev), ns,
                                     want_list=False)
        act, rlen, d_lst, cnt = wc.rx_reply_plan(d_buf, d_off, d_len, v, sock, d_eng, slot)
        self.verdict = v.cpu().numpy()
        self.sock = sock.cpu().numpy() if with_sock else None
        self.action, self.reply_len = act.cpu().numpy(), rlen.cpu().numpy()
        self.count = int(cnt.item())
        self.list = d_lst.cpu().numpy().view(np.uint32)[:self.count]
        self.m = self.count + 5 if m is None else m
        self.out0, self.out_offs = cases.out_slots(self.m, slot, rng)
        self.ip_ids = rng.integers(0, 1 << 16, self.m).astype(np.uint16) if ip_ids else None
        d_out = torch.from_numpy(self.out0.copy()).to(dev)
        if action is not None:  # a stale action array / another list
            act = torch.from_numpy(action).to(dev)
        if lst is not None:
            d_lst = torch.from_numpy(lst.view(np.int32)).to(dev)
            cnt = torch.tensor([len(lst)], dtype=torch.int64, device=dev)
        olen, built = wc.rx_reply_build(
            d_buf, d_off, d_len, act, d_lst, cnt, d_eng, d_out, torch.from_numpy(self.out_offs).to(dev),
            slot, None if self.ip_ids is None else torch.from_numpy(self.ip_ids).to(dev))
        torch.cuda.synchronize()
        self.out, self.out_len, self.built = d_out.cpu().numpy(), olen.cpu().numpy(), int(built.item())
        self.rx_after = d_buf.cpu().numpy()

    def check(self, frames=None, action=None, lst=None):
        if frames is not None:  # the calls in front gave what the oracle and the cases say
            assert (self.verdict == cases.verdicts_of(frames)).all()
            if self.sock is not None:
                assert (self.sock == cases.socks_of(frames)).all()
        ex = model.Expect(self.buf, self.offs, self.lens, self.verdict, self.sock, self.eng, self.slot)
        bad = np.flatnonzero(self.action != ex.action)
        assert bad.size == 0, (bad[:8], self.action[bad[:8]], ex.action[bad[:8]])
        assert (self.reply_len == ex.reply_len).all()
        assert self.count == len(ex.list) and (self.list == ex.list).all()
        out, out_len, built = ex.built(self.out0, self.out_offs, self.ip_ids, action, lst)
        assert (self.out_len == out_len).all() and self.built == built
        diff = np.flatnonzero(self.out != out)
        assert diff.size == 0, f"{diff.size} output bytes differ, the first at {diff[:4]}"
        assert (self.rx_after == self.buf).all()
        return ex


def layout(name, frames, seed):
    rng = np.random.default_rng(seed)
    return cases.slots(frames, rng) if name == "slots" else cases.packed(frames, rng, seed % 16)


@pytest.mark.parametrize("name", ["slots", "packed"])
def test_world(gpu, socktab, name):
    seed, n, slot = cases.WORLDS[name]
    frames = cases.world(seed, n)
    eng = cases.engine_table(rng=np.random.default_rng(seed))
    buf, offs, lens = layout(name, frames, seed)
    a = Run(gpu, socktab, buf, offs, lens, eng, slot, ip_ids=True)
    ex = a.check(frames)
    assert set(ex.action.tolist()) == set(model.ALL_ACTIONS)  # the census, on the device's verdicts
    b = Run(gpu, socktab, buf, offs, lens, eng, slot, ip_ids=True)  # the same input again
    assert (a.out == b.out).all() and (a.action == b.action).all() and (a.list == b.list).all()
    assert (a.out_len == b.out_len).all() and a.built == b.built


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_batches_and_every_m(gpu, socktab, n):
    frames = cases.world(300 + n, n)
    if n == 1:
        frames = [(cases.echo4(bytes(range(77))), None)]
    eng = cases.engine_table()
    for k, name in enumerate(("slots", "packed")):
        buf, offs, lens = layout(name, frames, n + k)
        r = Run(gpu, socktab, buf, offs, lens, eng, 2048, seed=n)
        r.check(frames)
        assert r.count > 0
        for m in {0, r.count - 1, r.count, r.count + 5}:
            Run(gpu, socktab, buf, offs, lens, eng, 2048, m=m, seed=m, ip_ids=bool(m & 1)).check()


def echo_frames(lens, rng, mtu_over=()):
    frames = []
    for i, dl in enumerate(lens):
        d = rng.integers(0, 256, dl, dtype=np.uint8).tobytes()
        frames += [(cases.echo4(d), None), (cases.echo6(d), None),
                   (cases.echo4(d, ihl=(6, 10, 15)[i % 3], rng=rng), None)]
    for over in mtu_over:  # ip_len = mtu + over: the reply carries what fits the MTU
        frames += [(cases.echo4(bytes(1500 + over - 28)), None),
                   (cases.echo6(bytes(1460 + over - 8)), None)]
    return frames


@pytest.mark.parametrize("name", ["slots", "packed"])
def test_echo_lengths_header_lengths_and_phases(gpu, socktab, name):
    rng = np.random.default_rng(5)
    frames = echo_frames(ECHO_LENS, rng, mtu_over=(1, 1000))
    buf, offs, lens = cases.slots(frames, rng, slot=4096) if name == "slots" else \
        cases.packed(frames, rng, 3)
    for ids in (False, True):
        r = Run(gpu, socktab, buf, offs, lens, cases.engine_table(), 2048, ip_ids=ids, seed=ids)
        ex = r.check(frames)
        assert r.built == len(frames) and set(ex.action.tolist()) == {model.ECHO4, model.ECHO6}
    assert {int(o) % 16 for o in offs} == set(range(16)) and {int(o) & 1 for o in r.out_offs} == {0, 1}


def test_jumbo_echo(gpu, socktab):
    rng = np.random.default_rng(6)
    frames = echo_frames((8972, 8971), rng)
    frames += [(cases.echo4(bytes(9000 + 1 - 28)), None), (cases.echo6(bytes(8960 + 1000 - 8)), None)]
    buf, offs, lens = cases.packed(frames, rng, 7)
    r = Run(gpu, socktab, buf, offs, lens, cases.engine_table(mtu=9000), 9100)
    r.check(frames)
    assert r.built == len(frames) and int(r.out_len.max()) == 9014


def test_grid(gpu, socktab):
    groups = {}
    for g in cases.grid():
        groups.setdefault((g[3].tobytes(), g[4], g[2] is None), []).append(g)
    seen = set()
    for k, ((_, slot, no_sock), gs) in enumerate(groups.items()):
        frames = [(g[1], g[2]) for g in gs]
        buf, offs, lens = cases.packed(frames, np.random.default_rng(k), k)
        # the grid states the socket id itself: bound / unbound frames come from the real
        # demux where the frame is delivered at all
        r = Run(gpu, socktab, buf, offs, lens, gs[0][3], slot, with_sock=not no_sock, seed=k)
        r.check()
        for g, a, ln in zip(gs, r.action, r.reply_len):
            if no_sock or g[2] == model.SOCK_UNBOUND:
                assert (int(a), int(ln)) == (g[5], g[6]), g[0]
            seen.add(int(a))
    assert seen == set(model.ALL_ACTIONS)


def test_batch_without_a_reply_and_without_d_sock(gpu, socktab):
    rng = np.random.default_rng(9)
    frames = [(cases.eth(cases.udp_pkt(4, bytes(40), cases.PORT), 0x0800), 0) for _ in range(70)]
    buf, offs, lens = cases.slots(frames, rng)
    r = Run(gpu, socktab, buf, offs, lens, cases.engine_table(), 2048, m=6)
    r.check(frames)
    assert r.count == 0 and r.built == 0 and (r.out == r.out0).all() and not r.out_len.any()
    # unbound frames from our own address: port unreachables with d_sock, nothing without
    seed, n, slot = cases.WORLDS["slots"]
    frames = cases.world(seed, 200)
    buf, offs, lens = cases.slots(frames, rng)
    with_sock = Run(gpu, socktab, buf, offs, lens, cases.engine_table(), 2048)
    without = Run(gpu, socktab, buf, offs, lens, cases.engine_table(), 2048, with_sock=False)
    with_sock.check(frames), without.check(frames)
    ports = (model.UNREACH_PORT4, model.UNREACH_PORT6)
    assert np.isin(with_sock.action, ports).any() and not np.isin(without.action, ports).any()


def test_stale_action_array(gpu, socktab):
    """The plan's actions shuffled against the frames, and a list with indices
    past the batch: every entry is length 0 or that action's reply, and
    nothing outside the slots is written (the whole buffer is compared)."""
    seed, n, slot = cases.WORLDS["packed"]
    frames = cases.world(seed, 300)
    buf, offs, lens = cases.packed(frames, np.random.default_rng(1), 5)
    eng = cases.engine_table()
    first = Run(gpu, socktab, buf, offs, lens, eng, slot)
    first.check(frames)
    rng = np.random.default_rng(2)
    for k in range(3):
        stale = first.action[rng.permutation(len(frames))].copy()
        stale[rng.integers(0, len(frames), 10)] = rng.integers(0, 256, 10)
        lst = np.concatenate([first.list, rng.integers(0, len(frames), 40).astype(np.uint32),
                              np.array([len(frames), len(frames) + 7, 0xFFFFFFFF], np.uint32)])
        rng.shuffle(lst)
        r = Run(gpu, socktab, buf, offs, lens, eng, slot, m=len(lst), action=stale, lst=lst, seed=k)
        r.check(action=stale, lst=lst)
        assert 0 < r.built < len(lst)


def test_replies_read_back_on_the_device(gpu, socktab):
    seed, n, slot = cases.WORLDS["slots"]
    frames = cases.world(seed, n)
    buf, offs, lens = cases.slots(frames, np.random.default_rng(4))
    r = Run(gpu, socktab, buf, offs, lens, cases.engine_table(), 2048)
    r.check(frames)
    keep = np.flatnonzero(r.out_len)
    assert keep.size == r.built > 50
    d_out = torch.from_numpy(r.out).to(gpu)
    d_off = torch.from_numpy(r.out_offs[keep]).to(gpu)
    d_len = torch.from_numpy(r.out_len[keep]).to(gpu)
    v, _ = wc.rx_verdict_ragged(d_out, d_off, d_len)
    act, rlen, _, cnt = wc.rx_reply_plan(d_out, d_off, d_len, v, None, dev_bytes(cases.peer_table(), gpu),
                                         2048)
    assert (v.cpu().numpy() == wc.RX_NOT_UDP).all()
    assert (act.cpu().numpy() == wc.RR_NONE).all() and not rlen.cpu().numpy().any()
    assert int(cnt.item()) == 0
