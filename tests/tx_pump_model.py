"""What wc_tx_pump must leave, from the existing models alone: tx_neigh_model's
resolve, hold and built for the destination side, the lists and the
solicitations, tx_build_model for the READY frames, and the contract's own
constants (wc_cksum.h, "TX pump") for the others -- a HELD frame is untouched,
has length 0 and status PUMP_HELD and is no error; a MALFORMED one is untouched,
WC_TX_MALFORMED and an error.  Nothing here reads warpcore_amd/csrc."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import tx_build_model as bmodel
import tx_neigh_model as nmodel

PUMP_HELD = 0x80  # WC_TX_PUMP_HELD
SMALL, SMALL_DST = 4096, 4096
READY, MALFORMED, HELD = nmodel.TH_READY, nmodel.TH_MALFORMED, nmodel.TH_HELD


def gate(hold: int, build_status: int, flen: int):
    """(status, frame_len, built, error) of one frame: its hold code, and the
    status and length the build alone gives it."""
    if hold == HELD:
        return PUMP_HELD, 0, False, False
    if hold != READY:
        return bmodel.MALFORMED, 0, False, True
    ok = build_status <= bmodel.SEALED_ZERO_UDP
    return build_status, flen if ok else 0, ok, not ok


def expect(cache: dict, dsts, afs, descs, socks, buf, offs, slot_bytes: int, zero_udp: bool, eng,
           sol_out, sol_offs, sol_slot: int):
    """Every output of one call.  dsts / descs / socks: structured arrays (dsts
    may be empty); buf / sol_out: the byte buffers before the call."""
    e = SimpleNamespace()
    dsts = np.asarray(dsts).reshape(-1).view(nmodel.DST).reshape(-1)
    descs = np.asarray(descs).reshape(-1).view(nmodel.DESC).reshape(-1)
    n, ndst = descs.size, dsts.size
    e.n, e.ndst, e.m = n, ndst, len(sol_offs)
    e.state, e.dsts, e.miss_list = nmodel.resolve(cache, dsts, afs)
    e.hold, e.held_list = nmodel.hold(descs, socks, e.state if ndst else None, afs)
    e.sol_out, e.sol_len, e.sol_built = nmodel.built(sol_out, sol_offs, sol_slot, e.dsts, afs,
                                                     e.miss_list, len(e.miss_list), eng)
    # the build of the READY frames alone, with the MACs resolve wrote
    ready = np.flatnonzero(e.hold == READY)
    b = bmodel.Expect(buf, np.asarray(offs)[ready], descs[ready], socks, e.dsts, slot_bytes, zero_udp)
    e.buf = b.buf
    e.status = np.where(e.hold == HELD, PUMP_HELD, bmodel.MALFORMED).astype(np.uint8)
    e.frame_len, e.ip_hdr, e.udp = (np.zeros(n, np.uint16) for _ in range(3))
    e.status[ready], e.frame_len[ready] = b.status, b.frame_len
    e.ip_hdr[ready], e.udp[ready] = b.ip_hdr, b.udp
    e.errors = b.errors + int((e.hold == MALFORMED).sum())
    # what the build alone would have said of every frame (the census reads it)
    e.ungated = np.array([bmodel.status_of(d, socks, ndst, slot_bytes, zero_udp) for d in descs],
                         np.uint8)
    return e
