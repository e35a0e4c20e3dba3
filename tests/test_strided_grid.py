"""CPU tests of tests/strided_grid.py: the grid is what it claims to be -- the
same in every process, a case in every (threshold, side, phase, stride class)
cell, inside the reference's domain -- and its expectations are the oracle's
(the C restatement against the byte-loop one here, both against the
reference's own object in tests/test_reference.py)."""
import subprocess
import sys
from pathlib import Path

import numpy as np

import strided_grid as sg
from oracle import c_oracle, py_oracle

TESTS = Path(__file__).resolve().parent


def test_case_count_and_census():
    cases = sg.grid()
    keys = [(c.length, c.stride, c.phase, c.n) for c in cases]
    assert len(set(keys)) == len(keys) == 10298
    assert len(sg.groups(cases)) == 2592
    assert len(sg.THRESHOLDS) == 28 and set(sg.SHAPE_T + sg.SEG_T + sg.SEG_ROWS_T + sg.LEAN_T) \
        <= set(sg.THRESHOLDS)
    c = sg.census(cases)
    want = sg.expected_cells()
    assert len(want) == (28 * 2 * 6 + 7 * 5) * 9
    assert set(c) == want
    assert min(c.values()) >= 2  # every cell at more than one n
    # every cell of a threshold with a batch below and at the seg route's n
    for t in sg.THRESHOLDS:
        ns = {case.n for case in sg.for_threshold(t)}
        assert {1, 63, 64} <= ns and max(ns) % 2 == 1 and max(ns) > 64
    # the sides stand where they say: the chunk count of the case's own phase
    for case in cases:
        for t, where, side, phase, _ in case.cells:
            if not isinstance(t, int):
                continue
            assert phase == case.phase
            assert sg.chunks(case.length, phase) == t + (where == "above")
            assert (side == "exact") == (phase == 0 and case.length % 16 == 0)
            assert (side == "head") == (phase != 0)
            assert (phase + case.length) % 16 == (15 if side == "tail" else 0)
    # no buffer passes a few MB
    assert max((c.n - 1) * c.stride + c.length for c in cases) < 3 << 20


def test_stride_classes():
    s = sg.strides_for(1000, 63)
    assert {k: v for k, v in s.items()} == {
        1000: ["len"], 1001: ["len+1"], 1125: ["len+len/8"], 1126: ["len+len/8+1"],
        1008: ["mult16"], 1024: ["mult64"], 2000: ["sparse-16"], 2016: ["sparse"],
        2048: ["slot"]}
    # a length that is its own multiple of 64 stands for three classes at once
    assert sg.strides_for(1024, 64)[1024] == ["len", "mult16", "mult64"]
    assert 2048 * 2 in sg.strides_for(2040, 128)  # the slot leaves 16 bytes for the phase


def test_grid_is_deterministic():
    """The same cases and the same bytes in another process."""
    code = ("import sys, zlib; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            "import strided_grid as sg\n"
            "g = sg.grid()\n"
            "pick = [g[i] for i in range(0, len(g), 997)] + list(sg.short_header_cases()[::97])\n"
            "print(zlib.crc32(repr(g).encode()),\n"
            "      *[zlib.crc32((sg.buffer(c) if hasattr(c, 'cells') else sg.short_buffer(c))"
            ".tobytes()) for c in pick])\n")
    runs = [subprocess.run([sys.executable, "-c", code, str(TESTS.parent), str(TESTS)], check=True,
                           capture_output=True, text=True).stdout for _ in range(2)]
    assert runs[0] == runs[1] and len(runs[0].split()) > 10


def test_buffers_are_random_and_never_zero():
    for case in sg.groups(sg.for_threshold(16))[::7] + sg.groups(sg.for_threshold("extra"))[::5]:
        buf = sg.buffer(case)
        assert buf.size == case.phase + (case.n - 1) * case.stride + max(case.length, 20) + sg.TAIL
        planted = np.zeros(buf.size, bool)
        if case.length:
            for o in case.offs.astype(np.int64):
                planted[o:o + min(case.length, 20)] = True  # the header fields may hold a 0
        assert (buf[~planted] != 0).all()
        if buf.size > 4000:
            assert np.unique(buf).size == 255 + bool((buf == 0).any())


def test_a_mask_one_byte_off_changes_every_result():
    """What the never-zero bytes are for: ip_cksum over a range that ends one
    byte later or earlier differs from the expectation in every packet (a
    byte of 1..255 added to either half of a word is never 0 mod 0xFFFF),
    whatever lies there: the tail, the gap to the next packet or the next
    packet itself."""
    cases = sg.groups(sg.grid())
    rng = np.random.default_rng(sg.SEED + 1)
    checked = 0
    for case in [cases[i] for i in rng.choice(len(cases), 150, replace=False)]:
        if not 2 <= case.length < 0xFFFF:
            continue
        buf, want = sg.buffer(case), sg.expect(case)["ip"]
        # (a planted header field or a random first byte may be 0: a packet
        # whose changed byte is one of those is not counted)
        planted = {int(o) + k for o in case.offs.astype(np.int64) for k in (0, 2, 3, 4, 5, 6, 7, 9)}
        for d_len in (1, -1):
            got = c_oracle.cksum_ragged(buf, case.offs, np.full(case.n, case.length + d_len,
                                                                np.uint16), kind=0)
            at = case.offs.astype(np.int64) + (case.length if d_len > 0 else case.length - 1)
            free = np.array([int(a) not in planted for a in at])
            assert (got != want)[free].all(), (case[:4], d_len)
            checked += int(free.sum())
    assert checked > 10000


def test_payload_cases_stay_inside_the_reference_domain():
    """len >= hl for every packet of every case that has the payload kinds,
    and the header kinds are all there."""
    seen = set()
    for case in sg.groups(sg.grid()):
        if "payload" not in case.kinds:
            assert case.length == 0
            continue
        first = sg.buffer(case)[case.offs.astype(np.int64)]
        assert (sg.hdr_len(first) <= case.length).all(), case[:4]
        if case.length >= 60 and case.n > 64:
            v4 = first >> 4 == 4
            ihl = first[v4] & 0x0F
            assert set(range(16)) <= set(ihl.tolist()), case[:4]
            assert (~v4).sum() >= case.n // 4
            seen |= set(first.tolist())
    assert len(seen) > 100  # the random first bytes


def test_c_oracle_equals_py_oracle_on_a_sample():
    rng = np.random.default_rng(sg.SEED)
    cases = sg.grid()
    pick = [cases[i] for i in rng.choice(len(cases), 120, replace=False)]
    pick += [c for c in sg.for_threshold("extra") if c.length == 65535 and c.n == 3][:2]
    for case in pick:
        buf, want = sg.buffer(case), sg.expect(case)
        assert set(want) == ({"ip", "payload", "hdr"} if case.length else {"ip"})
        for i in sorted({0, case.n // 2, case.n - 1}):
            o = int(case.offs[i])
            pkt = buf[o:o + max(case.length, 40)].tobytes()
            assert py_oracle.ip_cksum(pkt[:case.length]) == int(want["ip"][i]), case[:4]
            if case.length:
                assert py_oracle.payload_cksum(pkt, case.length) == int(want["payload"][i]), case[:4]
                assert py_oracle.ip_hdr_cksum(pkt + bytes(24)) == int(want["hdr"][i]), case[:4]


def test_short_header_family():
    """20 <= len < hl, IHL 6..15, every phase, strides 64, 2048 and packed;
    the expected header checksums are ip_cksum(pkt, hl)."""
    cases = sg.short_header_cases()
    assert len(cases) == len(sg.SHORT_LENS) * 3 * len(sg.PHASES) * len(sg.N_SET) == 540
    assert {c.phase for c in cases} == set(sg.PHASES)
    ihls = set()
    for case in cases:
        buf, want = sg.short_buffer(case), sg.short_expect(case)
        assert case.stride in (case.length, 64, 2048)
        offs = case.offs.astype(np.int64)
        first = buf[offs]
        hl = (first & 0x0F).astype(np.int64) * 4
        assert (first >> 4 == 4).all() and (hl > case.length).all() and case.length >= 20
        assert int(offs[-1]) + 60 <= buf.size  # the whole header lies inside the buffer
        ihls |= set((hl // 4).tolist())
        for i in {0, case.n - 1, case.n // 3}:
            o = int(offs[i])
            assert int(want[i]) == c_oracle.ip_cksum(buf[o:o + int(hl[i])])
            assert int(want[i]) == py_oracle.ip_cksum(buf[o:o + int(hl[i])].tobytes())
    assert ihls == set(range(6, 16))
    # the example of the issue: IHL 15, len 24, phase 0 -- 2 chunks loaded of 4
    assert any(c.length == 24 and c.phase == 0 and
               (sg.short_buffer(c)[c.offs.astype(np.int64)] == 0x4F).any() for c in cases)
    pk = sg.short_packets()
    assert len(pk) > 600 and all(20 <= ln < len(b) == 4 * (b[0] & 15) for b, ln in pk)
    assert {b[0] & 15 for b, _ in pk} == set(range(6, 16))
