"""CPU census of the TX pump's census world (tests/tx_pump_cases.py, 600 frames
to 257 destinations): the expectation the GPU tests compare against holds at
least ten of every hold code, every resolve state, every status the gated build
can return -- each of them under READY --, and HELD frames that the build alone
would have sealed; and the model's own parts agree with each other."""
import numpy as np
import pytest

import tx_build_model as bmodel
import tx_neigh_model as nmodel
import tx_pump_cases as cases
import tx_pump_model as model

N, NDST = cases.CENSUS


@pytest.fixture(scope="module")
def both():
    w = cases.world(7, N, NDST)
    return w, cases.expect(w, False), cases.expect(w, True)


def test_census_of_the_base_world(both):
    w, e, z = both
    assert (e.n, e.ndst) == (600, 257)
    for code in (nmodel.TH_READY, nmodel.TH_MALFORMED, nmodel.TH_HELD):
        assert (e.hold == code).sum() >= 10, code
    for code in (nmodel.READY, nmodel.BAD_AF, nmodel.MISS, nmodel.MISS_DUP):
        assert (e.state == code).sum() >= 10, code
    ready = e.hold == nmodel.TH_READY
    for x, codes in ((e, (bmodel.SEALED, bmodel.MALFORMED, bmodel.TRUNCATED)),
                     (z, (bmodel.SEALED_ZERO_UDP, bmodel.MALFORMED, bmodel.TRUNCATED))):
        for code in codes:
            assert (x.status[ready] == code).sum() >= 10, code
    held = e.hold == nmodel.TH_HELD
    assert (held & (e.ungated == bmodel.SEALED)).sum() >= 10
    assert (e.status[held] == model.PUMP_HELD).all() and not e.frame_len[held].any()
    # what the worlds are said to hold
    assert {0, 7} <= set(w.afs.tolist()) and {4, 6} <= set(w.afs.tolist())
    assert (w.descs["dst"] == NDST).any() and (w.descs["dst"] > NDST).any()
    assert (w.descs["sock"] == len(w.socks)).any() and (w.descs["sock"] > len(w.socks)).any()
    assert {0, 1472}.issubset(w.descs["data_len"].tolist()) and (w.descs["data_len"] > w.slot).any()
    assert nmodel.BCAST in w.cache.values()
    bc_keys = {k for k, m in w.cache.items() if m == nmodel.BCAST}
    d = w.dsts
    assert any(nmodel.key(int(a), bytes(x)) in bc_keys for a, x in zip(w.afs, d["addr"]))
    # a destination family that is not the socket's: MALFORMED here, sealed by the build alone
    mal = e.hold == nmodel.TH_MALFORMED
    assert (mal & (e.ungated == bmodel.SEALED)).sum() >= 10
    assert len(e.miss_list) >= 10 and e.sol_built == len(e.miss_list) >= 10
    assert e.errors > 0 and e.errors == int((e.status > bmodel.SEALED_ZERO_UDP).sum()) - int(held.sum())


def test_untouched_frames_and_the_parts_agree(both):
    w, e, z = both
    for x in (e, z):
        for i in np.flatnonzero(x.frame_len == 0):
            o = int(w.offs[i])
            assert (x.buf[o:o + 62] == w.buf[o:o + 62]).all(), i
        # only header bytes of built frames differ from the input
        diff = np.flatnonzero(x.buf != w.buf)
        owner = np.searchsorted(np.sort(w.offs), diff, side="right") - 1
        order = np.argsort(w.offs)
        for at, k in zip(diff[:2000], owner[:2000]):
            i = order[k]
            assert x.frame_len[i] and at - int(w.offs[i]) < 62
    assert (z.udp == 0).all() and e.udp.any()
    assert (e.hold == z.hold).all() and (e.state == z.state).all()


def test_gate_grid():
    for st in (bmodel.SEALED, bmodel.SEALED_ZERO_UDP):
        assert model.gate(nmodel.TH_READY, st, 99) == (st, 99, True, False)
    for st in (bmodel.MALFORMED, bmodel.TRUNCATED):
        assert model.gate(nmodel.TH_READY, st, 99) == (st, 0, False, True)
    for st in (bmodel.SEALED, bmodel.SEALED_ZERO_UDP, bmodel.MALFORMED, bmodel.TRUNCATED):
        assert model.gate(nmodel.TH_HELD, st, 99) == (model.PUMP_HELD, 0, False, False)
        assert model.gate(nmodel.TH_MALFORMED, st, 99) == (bmodel.MALFORMED, 0, False, True)


@pytest.mark.parametrize("n,ndst", [(0, 257), (600, 0), (0, 0), (1, 1)])
def test_empty_sides(n, ndst):
    w = cases.world(3, n, ndst, connected_only=ndst == 0)
    e = cases.expect(w)
    assert len(e.state) == ndst and len(e.hold) == n and len(e.sol_len) == w.m
    if ndst == 0:
        assert e.sol_built == 0 and not e.sol_len.any() and len(e.held_list) == 0
        assert (e.hold == nmodel.TH_READY).all()
    if n == 0:
        assert e.errors == 0 and (e.buf == w.buf).all()
