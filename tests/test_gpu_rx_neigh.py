"""GPU tests of the RX neighbours (wc_rx_neigh_plan, wc_rx_neigh_updates,
wc_rx_neigh_build) against tests/rx_neigh_model.py, through the real
rx_verdict_ragged -> rx_reply_plan -> rx_neigh_plan -> rx_neigh_updates /
rx_neigh_build: codes, both lists and counts, the records, out lengths, the
built count, the whole output buffer (random fill, gaps and guard bytes
included) and the whole RX buffer, all exact."""
import numpy as np
import pytest
import torch

import rx_neigh_cases as cases
import rx_neigh_model as model
import rx_reply_cases as rc
import rx_reply_model as rmodel
import warpcore_amd as wc

pytestmark = pytest.mark.gpu


def dev_bytes(a: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def dev_list(lst: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(lst, np.uint32).view(np.int32).copy()).to(dev)


class Run:
    """One batch through the five calls; every result on the host.  frames:
    the cases' triples, whose forced action bytes overwrite the reply plan's;
    m_upd / m_out: entries asked of the two list calls (default: count + 5);
    nact / ulist / rlist: other arrays than the plan's own for the list calls."""

    def __init__(self, dev, frames, buf, offs, lens, eng, slot=2048, m_upd=None, m_out=None, seed=0,
                 nact=None, ulist=None, rlist=None, phased=True):
        rng = np.random.default_rng(2000 + seed)
        self.frames, self.buf, self.offs, self.lens, self.eng, self.slot = frames, buf, offs, lens, eng, slot
        d_buf = torch.from_numpy(buf.copy()).to(dev)
        d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
        d_eng = dev_bytes(eng, dev)
        v, _ = wc.rx_verdict_ragged(d_buf, d_off, d_len)
        act, _, _, _ = wc.rx_reply_plan(d_buf, d_off, d_len, v, None, d_eng, 2048, want_list=False)
        self.verdict, self.real = v.cpu().numpy(), act.cpu().numpy()
        self.action = cases.actions_of(frames, eng, real=self.real)
        d_act = torch.from_numpy(self.action).to(dev)
        d_nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(d_buf, d_off, d_len, d_act, d_eng)
        self.nact = d_nact.cpu().numpy()
        self.rcount, self.ucount = int(rcnt.item()), int(ucnt.item())
        self.rlist = rl.cpu().numpy().view(np.uint32)[:self.rcount]
        self.ulist = ul.cpu().numpy().view(np.uint32)[:self.ucount]
        if nact is not None:  # a stale code array / other lists
            d_nact = torch.from_numpy(nact).to(dev)
        if ulist is not None:
            ul, ucnt = dev_list(ulist, dev), torch.tensor([len(ulist)], dtype=torch.int64, device=dev)
        if rlist is not None:
            rl, rcnt = dev_list(rlist, dev), torch.tensor([len(rlist)], dtype=torch.int64, device=dev)
        self.m_upd = self.ucount + 5 if m_upd is None else m_upd
        self.m_out = self.rcount + 5 if m_out is None else m_out
        upd = wc.rx_neigh_updates(d_buf, d_off, d_len, d_nact, ul, ucnt, self.m_upd)
        self.out0, self.out_offs = rc.out_slots(self.m_out, slot, rng, phased)
        d_out = torch.from_numpy(self.out0.copy()).to(dev)
        olen, built = wc.rx_neigh_build(d_buf, d_off, d_len, d_nact, rl, rcnt, d_eng, d_out,
                                        torch.from_numpy(self.out_offs).to(dev), slot)
        torch.cuda.synchronize()
        self.upd = upd.cpu().numpy()
        self.out, self.out_len, self.built = d_out.cpu().numpy(), olen.cpu().numpy(), int(built.item())
        self.rx_after = d_buf.cpu().numpy()

    def check(self, nact=None, ulist=None, rlist=None):
        # the calls in front gave what the oracle and the reply model say
        pairs = [(f[0], f[1]) for f in self.frames]
        assert (self.verdict == rc.verdicts_of(pairs)).all()
        want = [rmodel.plan(fr, int(self.verdict[i]), None, self.eng, 2048)[0]
                for i, (fr, _) in enumerate(pairs)]
        assert (self.real == np.array(want, np.uint8).reshape(len(pairs))).all()
        ex = model.Expect(self.buf, self.offs, self.lens, self.action, self.eng)
        bad = np.flatnonzero(self.nact != ex.nact)
        assert bad.size == 0, (bad[:8], self.nact[bad[:8]], ex.nact[bad[:8]])
        assert self.rcount == len(ex.rlist) and (self.rlist == ex.rlist).all()
        assert self.ucount == len(ex.ulist) and (self.ulist == ex.ulist).all()
        upd = ex.updates(self.m_upd, nact, ulist)
        bad = np.flatnonzero((self.upd != upd).any(axis=1))
        assert bad.size == 0, (bad[:4], self.upd[bad[:4]], upd[bad[:4]])
        out, out_len, built = ex.built(self.out0, self.out_offs, self.slot, nact, rlist)
        assert (self.out_len == out_len).all() and self.built == built
        diff = np.flatnonzero(self.out != out)
        assert diff.size == 0, f"{diff.size} output bytes differ, the first at {diff[:4]}"
        assert (self.rx_after == self.buf).all()
        return ex


@pytest.mark.parametrize("name", list(cases.WORLDS))
def test_world(gpu, name):
    seed, n = cases.WORLDS[name]
    frames = cases.world(seed, n)
    buf, offs, lens = cases.layout(name, frames, seed)
    eng = rc.engine_table(rng=np.random.default_rng(seed))
    a = Run(gpu, frames, buf, offs, lens, eng)
    c = a.check().census()
    assert set(c) == set(cases.CENSUS) and min(c.values()) >= 10  # on the device's actions
    b = Run(gpu, frames, buf, offs, lens, eng)  # the same input again
    assert (a.nact == b.nact).all() and (a.rlist == b.rlist).all() and (a.ulist == b.ulist).all()
    assert (a.upd == b.upd).all() and (a.out == b.out).all() and (a.out_len == b.out_len).all()
    assert a.built == b.built == a.rcount
    no4 = Run(gpu, frames, buf, offs, lens, rc.engine_table(v4=0), seed=1)
    assert no4.check().census()[(model.NONE, "no ip4")] >= 10


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_batches_and_every_m(gpu, n):
    frames = cases.world(500 + n, n)
    if n == 1:
        frames = [(bytes.fromhex(cases.NSOL_HEX), None, None)]
    eng = rc.engine_table()
    for k, name in enumerate(("slots", "packed")):
        buf, offs, lens = cases.layout(name, frames, n + k)
        r = Run(gpu, frames, buf, offs, lens, eng, seed=n)
        r.check()
        assert r.rcount > 0 and r.ucount >= r.rcount
        for mu, mo in zip((0, r.ucount - 1, r.ucount, r.ucount + 1),
                          (0, r.rcount - 1, r.rcount, r.rcount + 1)):
            Run(gpu, frames, buf, offs, lens, eng, m_upd=mu, m_out=mo, seed=mu).check()


def test_known_answers(gpu):
    frames = [(bytes.fromhex(cases.NSOL_HEX), None, None), (bytes.fromhex(cases.ARP_HEX), None, None)]
    buf, offs, lens = cases.layout("packed", frames, 5)
    r = Run(gpu, frames, buf, offs, lens, rc.engine_table(), m_upd=2, m_out=2)
    r.check()
    got = [r.out[int(o):int(o) + int(ln)].tobytes().hex() for o, ln in zip(r.out_offs, r.out_len)]
    assert got == [cases.NADV_HEX, cases.IS_AT_HEX]
    u = r.upd.view(model.UPDATE).reshape(-1)
    assert u["af"].tolist() == [6, 4] and u["action"].tolist() == [model.NADV, model.ARP_IS_AT]
    assert bytes(u["mac"][0]) == bytes(u["mac"][1]) == rc.PEER_MAC
    assert bytes(u["addr"][0]) == rc.PEER6 and bytes(u["addr"][1]) == rc.PEER4 + bytes(12)


def test_grid(gpu):
    groups = {}
    for g in cases.grid():
        groups.setdefault(g[3].tobytes(), []).append(g)
    seen = set()
    for k, gs in enumerate(groups.values()):
        # the grid states the action byte itself: forced on top of the real plan's
        frames = [(g[1], None, g[2]) for g in gs]
        buf, offs, lens = cases.layout("packed", frames, k + 3)
        r = Run(gpu, frames, buf, offs, lens, gs[0][3], seed=k)
        r.check()
        for g, c in zip(gs, r.nact):
            assert int(c) == g[4], g[0]
            seen.add(int(c))
    assert seen == set(model.ALL_ACTIONS)


def test_batch_without_a_host_frame_and_an_empty_batch(gpu):
    rng = np.random.default_rng(9)
    frames = [(rc.eth(rc.udp_pkt(4, bytes(40), rc.PORT), 0x0800), 0, None) for _ in range(70)]
    buf, offs, lens = rc.slots([(f[0], f[1]) for f in frames], rng)
    r = Run(gpu, frames, buf, offs, lens, rc.engine_table(), m_upd=6, m_out=6)
    r.check()
    assert r.rcount == r.ucount == r.built == 0 and not r.nact.any()
    assert (r.out == r.out0).all() and not r.out_len.any() and not r.upd.any()
    # n = 0: zero counts, zero records, zero lengths
    e = torch.zeros(0, dtype=torch.uint8, device=gpu)
    o = torch.zeros(0, dtype=torch.int64, device=gpu)
    ln = torch.zeros(0, dtype=torch.uint16, device=gpu)
    d_eng = dev_bytes(rc.engine_table(), gpu)
    nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(e, o, ln, e, d_eng)
    rcnt.fill_(7), ucnt.fill_(7)
    nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(e, o, ln, e, d_eng)
    assert int(rcnt.item()) == int(ucnt.item()) == 0
    lst = torch.zeros(4, dtype=torch.int32, device=gpu)
    cnt = torch.tensor([3], dtype=torch.int64, device=gpu)
    upd = wc.rx_neigh_updates(e, o, ln, e, lst, cnt, 3)
    out = torch.full((512,), 0xA5, dtype=torch.uint8, device=gpu)
    olen, built = wc.rx_neigh_build(e, o, ln, e, lst, cnt, d_eng, out,
                                    torch.tensor([0, 100, 200], dtype=torch.int64, device=gpu), 86)
    assert not upd.cpu().numpy().any() and not olen.cpu().numpy().any() and int(built.item()) == 0
    assert (out.cpu().numpy() == 0xA5).all()


@pytest.mark.parametrize("slot", [41, 42, 85, 86, 87])
def test_slot_bytes_and_slots_at_every_phase(gpu, slot):
    frames = cases.world(77, 200)
    buf, offs, lens = cases.layout("packed", frames, slot)
    r = Run(gpu, frames, buf, offs, lens, rc.engine_table(), slot=slot, seed=slot)
    ex = r.check()
    lens_seen = set(r.out_len.tolist())
    assert lens_seen == {0} | ({42} if slot >= 42 else set()) | ({86} if slot >= 86 else set())
    assert {int(o) % 4 for o, ln in zip(r.out_offs, r.out_len) if ln == 42} == \
        ({0, 1, 2, 3} if slot >= 42 else set())
    assert {int(o) % 4 for o, ln in zip(r.out_offs, r.out_len) if ln == 86} == \
        ({0, 1, 2, 3} if slot >= 86 else set())
    assert len(ex.rlist) > 20


def test_stale_codes_and_indices_past_the_batch(gpu):
    """The plan's codes shuffled against the frames and lists with indices past
    n: every entry is an empty record / length 0 or that code's record / reply,
    and nothing outside the slots is written (the whole buffer is compared)."""
    seed, n = cases.WORLDS["packed"]
    frames = cases.world(seed, 300)
    buf, offs, lens = cases.layout("packed", frames, 5)
    eng = rc.engine_table()
    first = Run(gpu, frames, buf, offs, lens, eng)
    first.check()
    rng = np.random.default_rng(2)
    for k in range(3):
        stale = first.nact[rng.permutation(len(frames))].copy()
        stale[rng.integers(0, len(frames), 10)] = rng.integers(0, 256, 10)
        lst = np.concatenate([first.ulist, rng.integers(0, len(frames), 40).astype(np.uint32),
                              np.array([len(frames), len(frames) + 7, 0xFFFFFFFF], np.uint32)])
        rng.shuffle(lst)
        r = Run(gpu, frames, buf, offs, lens, eng, m_upd=len(lst), m_out=len(lst), nact=stale,
                ulist=lst, rlist=lst, seed=k)
        r.check(nact=stale, ulist=lst, rlist=lst)
        assert 0 < r.built < len(lst) and 0 < r.upd.any(axis=1).sum() < len(lst)


def test_replies_fed_back_with_the_peers_table(gpu):
    frames = cases.peer_requests()
    buf, offs, lens = cases.layout("slots", frames, 4)
    eng, peer = rc.engine_table(), rc.peer_table()
    r = Run(gpu, frames, buf, offs, lens, eng, m_out=len(frames), m_upd=len(frames))
    r.check()
    assert r.built == len(frames) and (r.out_len != 0).all()
    d_out = torch.from_numpy(r.out).to(gpu)
    d_off, d_len = torch.from_numpy(r.out_offs).to(gpu), torch.from_numpy(r.out_len).to(gpu)
    d_peer = dev_bytes(peer, gpu)
    v, _ = wc.rx_verdict_ragged(d_out, d_off, d_len)
    act, _, _, _ = wc.rx_reply_plan(d_out, d_off, d_len, v, None, d_peer, 2048, want_list=False)
    assert (act.cpu().numpy() == wc.RR_HOST).all()
    nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(d_out, d_off, d_len, act, d_peer)
    upd = wc.rx_neigh_updates(d_out, d_off, d_len, nact, ul, ucnt, len(frames))
    u = upd.cpu().numpy().view(model.UPDATE).reshape(-1)
    assert int(rcnt.item()) == 0 and int(ucnt.item()) == len(frames)
    for j, (fr, _, _) in enumerate(frames):
        arp = fr[12:14] == b"\x08\x06"
        assert int(nact[j].item()) == (wc.RN_UPDATE4 if arp else wc.RN_UPDATE6)
        assert int(u["af"][j]) == (4 if arp else 6) and bytes(u["mac"][j]) == rc.MAC
        assert bytes(u["addr"][j]) == (fr[38:42] + bytes(12) if arp else fr[62:78])
