"""The boundary grid of tests/rx_edges.py through all four device copies of
the decision chain: rx_decide behind the one-round and the two-round parse
(wc_rx_verdict_ragged, wc_rx_deliver_ragged with rx_record on top), sv_rx in
the resident server (wc_rx_verdict_host on a registered ring) and tx_decide
(wc_tx_seal_ragged).  Every frame stands on, one below or one above a
threshold of the chain (test_rx_edges.py holds the census), and every
comparison is exact: verdict, drop count, all 16 record bytes, the list, the
status, both values and the whole buffer after a seal.

Layouts: scrambled 128-byte slots, each holding the frame and what was cut off
it (the bytes that would turn TRUNCATED into OK if a load read them), and the
frames back to back -- the next frame's Ethernet header right behind a cut
one -- shifted to every start phase 0..15 of a 16-byte chunk.  A frame's
verdict, record and seal depend on its bytes alone, so each expectation is
computed once and shared by every layout and kernel mode.
"""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rx_deliver_model
import rx_edges
import tx_model
import warpcore_amd as wc
from test_gpu_rx import RX_MODES as VERDICT_MODES
from test_gpu_rx_deliver import RX_MODES as DELIVER_MODES
from test_gpu_rx_deliver import run_deliver

pytestmark = pytest.mark.gpu

LAYOUTS = ("slots",) + tuple(f"phase{p}" for p in range(16))


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.array(a, copy=True)).to(d)  # (the shared layouts are read-only)


def lay_out(frames) -> dict:
    """name -> (buf, offs, lens) of `frames` in every layout, read-only."""
    out = {"slots": rx_edges.slots(frames)}
    for p in range(16):
        out[f"phase{p}"] = rx_edges.packed(frames, p)
        assert int(out[f"phase{p}"][1][0]) == p
    for arrays in out.values():
        for a in arrays:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def rx():
    """The grid, its RX expectation (oracle verdicts, model records, list,
    drops) and its layouts on the host."""
    frames = rx_edges.grid()
    r = SimpleNamespace(frames=frames, exp=rx_deliver_model.Expect(*rx_edges.packed(frames)),
                        layouts=lay_out(frames))
    assert set(np.unique(r.exp.verdicts).tolist()) == set(range(10))
    return r


@pytest.fixture(scope="module")
def rx_dev(rx, gpu):
    """The layouts on the device (the RX calls only read them)."""
    return {name: tuple(dev(a, gpu) for a in arrays) for name, arrays in rx.layouts.items()}


def set_mode(monkeypatch, env: dict):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wc.reload_config()


def clear_mode(monkeypatch, env: dict):
    for k in env:
        monkeypatch.delenv(k)
    wc.reload_config()


def first_difference(rx, name, got, want, what="verdict") -> str:
    bad = np.flatnonzero(got != want)
    fr, flen, tag = rx.frames[bad[0]]
    return (f"{name}: {bad.size} {what}s differ, first frame {bad[0]} {tag} (flen {flen}): "
            f"got {got[bad[0]]} want {want[bad[0]]}")


# --- verdicts -------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(VERDICT_MODES))
def test_edge_verdicts(gpu, rx, rx_dev, monkeypatch, mode):
    """wc_rx_verdict_ragged in every kernel mode over the slots and all 16
    phases: every verdict and the drop count exact."""
    set_mode(monkeypatch, VERDICT_MODES[mode])
    try:
        for name in LAYOUTS:
            got, drops = wc.rx_verdict_ragged(*rx_dev[name])
            got = got.cpu().numpy()
            assert np.array_equal(got, rx.exp.verdicts), \
                first_difference(rx, f"{mode} {name}", got, rx.exp.verdicts)
            assert int(drops.item()) == rx.exp.drops, (mode, name)
    finally:
        clear_mode(monkeypatch, VERDICT_MODES[mode])


# --- records --------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(DELIVER_MODES))
def test_edge_records(gpu, rx, monkeypatch, mode):
    """wc_rx_deliver_ragged: verdicts, all 16 record bytes (data_len's uint16
    wrap for udp_len < 8, OK_NO_CKSUM records whose data runs past the frame),
    the list, the count and the entries past it."""
    recs = rx.exp.records
    wrapped = recs["data_len"] >= 65528
    assert {wc.RX_OK, wc.RX_OK_NO_CKSUM} <= set(rx.exp.verdicts[wrapped].tolist())
    set_mode(monkeypatch, DELIVER_MODES[mode])
    try:
        for name in LAYOUTS:
            buf, offs, lens = (a.copy() for a in rx.layouts[name])  # (run_deliver wraps, not copies)
            try:
                run_deliver(buf, offs, lens, rx.exp, gpu)
            except AssertionError as e:
                raise AssertionError(f"{mode} {name}: {e}" + tags_of(rx, e)) from None
    finally:
        clear_mode(monkeypatch, DELIVER_MODES[mode])


def tags_of(rx, e: AssertionError) -> str:
    """The tags of the frame indices run_deliver's message lists after 'first'."""
    m = re.search(r"first \[([0-9 ]*)\]", str(e))
    if not m:
        return ""
    return "; frames " + ", ".join(f"{i}: {rx.frames[int(i)][2]}" for i in m.group(1).split())


# --- the resident server --------------------------------------------------------

def test_edge_verdicts_from_the_server(gpu, rx):
    """The grid in a registered host ring, asked for in consecutive batches
    of at most 256 frames: sv_rx answers every one (served grows by one per
    call, no fallback), every verdict and drop count exact.  Then the whole
    grid from pageable memory in one call (the launch path)."""
    buf, offs, lens = (a.copy() for a in rx.layouts["slots"])
    want = rx.exp.verdicts
    n = len(rx.frames)
    calls = 0
    wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        for lo in range(0, n, 256):
            hi = min(lo + 256, n)
            got, drops = wc.rx_verdict_host(buf, offs[lo:hi], lens[lo:hi])
            calls += 1
            assert np.array_equal(got, want[lo:hi]), "server, frames from %d: " % lo + \
                first_difference(rx, "server", np.concatenate((want[:lo], got, want[hi:])), want)
            assert drops == int(np.isin(want[lo:hi], wc.RX_DROPS).sum()), lo
    finally:
        wc.host_unregister(buf)
    s1 = wc.server_stats()
    assert calls == (n + 255) // 256
    assert (s1["served"] - s0["served"], s1["fallbacks"] - s0["fallbacks"]) == (calls, 0)
    got, drops = wc.rx_verdict_host(buf, offs, lens)
    assert np.array_equal(got, want), first_difference(rx, "pageable", got, want)
    assert drops == rx.exp.drops
    s2 = wc.server_stats()
    assert (s2["served"], s2["fallbacks"]) == (s1["served"], s1["fallbacks"])


# --- the seal -------------------------------------------------------------------

class SealExpect:
    """tx_model.Expect of the garbled grid, computed once on the packed frames
    and carried to any layout: a frame's stores are offsets from its start."""

    def __init__(self, frames, zero_udp: bool):
        buf, offs, lens = rx_edges.packed(frames)
        e = tx_model.Expect(buf, offs, lens, zero_udp=zero_udp)
        self.status, self.ip_hdr, self.udp, self.errors = e.status, e.ip_hdr, e.udp, e.errors
        st = [(i, at, v) for i, s in enumerate(e.seals) for at, v in s.stores]
        self.frame, self.at, self.val = (np.array(x, np.int64) for x in zip(*st))
        np.testing.assert_array_equal(self.buffer(buf, offs), e.buf)

    def buffer(self, buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
        want = buf.copy()
        pos = offs.astype(np.int64)[self.frame] + self.at
        # (two stores of one frame never share a byte: the fields are apart)
        want[pos] = self.val & 0xFF
        want[pos + 1] = self.val >> 8
        return want


@pytest.fixture(scope="module")
def tx():
    frames = rx_edges.garbled(rx_edges.grid())
    t = SimpleNamespace(frames=frames, layouts=lay_out(frames),
                        exp={z: SealExpect(frames, z) for z in (False, True)})
    plain, zero = t.exp[False].status, t.exp[True].status
    assert set(np.unique(plain).tolist()) | set(np.unique(zero).tolist()) == set(range(8))
    return t


def seal(buf, offs, lens, d, **kw):
    """Seal a device copy of exactly buf.size bytes; everything back on the host."""
    t = dev(buf, d)
    assert t.numel() == buf.size
    status, hdr, udp, errors = wc.tx_seal_ragged(t, dev(offs, d), dev(lens, d), **kw)
    return (t.cpu().numpy(), status.cpu().numpy(), hdr.cpu().numpy(), udp.cpu().numpy(),
            int(errors.item()))


def assert_sealed(tx, name, got, e: SealExpect, want_buf):
    buf, status, hdr, udp, errors = got
    assert np.array_equal(status, e.status), first_difference(tx, name, status, e.status, "status code")
    assert np.array_equal(hdr, e.ip_hdr), first_difference(tx, name, hdr, e.ip_hdr, "header value")
    assert np.array_equal(udp, e.udp), first_difference(tx, name, udp, e.udp, "UDP value")
    assert errors == e.errors, name
    bad = np.flatnonzero(buf != want_buf)
    assert bad.size == 0, (f"{name}: {bad.size} bytes differ, first at {bad[:8]}: got "
                           f"{buf[bad[:8]]} want {want_buf[bad[:8]]}")


@pytest.mark.parametrize("zero_udp", [False, True])
def test_edge_seal(gpu, tx, zero_udp):
    """wc_tx_seal_ragged over the slots and all 16 phases: status, both
    values, the error count and the whole buffer.  A frame cut one byte short
    of its UDP header is TRUNCATED and not a byte of it is stored, the IPv4
    header checksum neither."""
    e = tx.exp[zero_udp]
    cut = np.array([tag.startswith("cut/") and rx_edges.frame_shape(fr) not in ("none", "other")
                    and flen == 14 + ((fr[14] & 15) * 4 if fr[14] >> 4 == 4 else 40) + 7
                    for fr, flen, tag in tx.frames])
    assert cut.sum() >= 6 * len(rx_edges.SHAPES) and (e.status[cut] == wc.TX_TRUNCATED).all()
    assert not np.isin(np.flatnonzero(cut), e.frame).any()
    for name in LAYOUTS:
        buf, offs, lens = tx.layouts[name]
        want = e.buffer(buf, offs)
        assert not np.array_equal(want, buf)
        got = seal(buf, offs, lens, gpu, zero_udp=zero_udp)
        assert_sealed(tx, f"zero_udp={zero_udp} {name}", got, e, want)
        for i in np.flatnonzero(cut).tolist():
            o = int(offs[i])
            assert np.array_equal(got[0][o:o + int(lens[i])], buf[o:o + int(lens[i])])


def test_edge_seal_no_store(gpu, tx):
    """store=False on the slots: the buffer unchanged, the values the same."""
    buf, offs, lens = tx.layouts["slots"]
    assert_sealed(tx, "store=False", seal(buf, offs, lens, gpu, store=False), tx.exp[False], buf)
