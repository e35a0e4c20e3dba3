"""CPU tests of the RX replies' C ABI (wc_rx_engine_check, wc_rx_reply_plan,
wc_rx_reply_build): the names are exported through the header, the library and
the Python mirror, the structs are 52 / 844 bytes, and every argument error
returns before a device is touched (there is no GPU here; the pointers are
poisoned)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rx_reply_cases as cases
import rx_reply_model as model
import warpcore_amd as wc
from warpcore_amd import _build, _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first


def test_reply_names_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    for name in ("wc_rx_engine_check", "wc_rx_reply_plan", "wc_rx_reply_build"):
        assert f" T {name}\n" in syms
        assert name in _lib.SIGNATURES
        assert re.search(rf"\bint {name}\(", text)
    for name in ("rx_engine_check", "rx_reply_plan", "rx_reply_build", "RX_IFADDR", "RX_ENGINE",
                 "RR_MASK_REPLY", "RR_ECHO4", "RR_UNREACH_PROTO4"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert "#define WC_RX_MAX_IFADDR 16" in text and wc.RX_MAX_IFADDR == 16
    assert "#define WC_RR_MASK_REPLY (0x1F00u)" in text and wc.RR_MASK_REPLY == model.MASK_REPLY
    for name, code in (("NONE", 0), ("HOST", 1), ("FILTERED", 2), ("ICMP_BAD_CKSUM", 3),
                       ("MALFORMED", 4), ("NO_ROOM", 5), ("ECHO4", 8), ("ECHO6", 9),
                       ("UNREACH_PORT4", 10), ("UNREACH_PORT6", 11), ("UNREACH_PROTO4", 12)):
        assert re.search(rf"\bWC_RR_{name} = {code}\b", text)
        assert getattr(wc, f"RR_{name}") == code == getattr(model, name)
    assert wc.RR_MASK_REPLY == sum(1 << a for a in model.REPLIES)


def test_struct_sizes_and_layouts(tmp_path):
    assert (wc.RX_IFADDR.itemsize, wc.RX_ENGINE.itemsize) == (52, 844)
    assert (wc.RX_IFADDR, wc.RX_ENGINE) == (model.IFADDR, model.ENGINE)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu\\n\", "
                   "sizeof(struct wc_rx_ifaddr), sizeof(struct wc_rx_engine), "
                   "offsetof(struct wc_rx_ifaddr, addr), offsetof(struct wc_rx_ifaddr, bcast), "
                   "offsetof(struct wc_rx_ifaddr, snma), offsetof(struct wc_rx_engine, mtu), "
                   "offsetof(struct wc_rx_engine, naddr), offsetof(struct wc_rx_engine, addr)); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [52, 844, 4, 20, 36, 6, 8, 12]
    f = wc.RX_IFADDR.fields
    assert (f["addr"][1], f["bcast"][1], f["snma"][1]) == (4, 20, 36)
    f = wc.RX_ENGINE.fields
    assert (f["mtu"][1], f["naddr"][1], f["addr"][1]) == (6, 8, 12)


def test_engine_check():
    lib = _lib.load()
    good = cases.engine_table()
    assert lib.wc_rx_engine_check(good.ctypes.data) == OK
    assert lib.wc_rx_engine_check(None) == EINVAL
    full = model.engine(cases.MAC, 68, [(6, cases.A6[0], cases.BC6, cases.SNMA6[0])] * 7 +
                        [(4, cases.A4[0], cases.BC4, None)] * 9)
    assert lib.wc_rx_engine_check(full.ctypes.data) == OK
    empty = model.engine(cases.MAC, 1500, [])
    assert lib.wc_rx_engine_check(empty.ctypes.data) == OK

    def refused(change):
        e = full.copy()
        change(e[0])
        return lib.wc_rx_engine_check(e.ctypes.data) == EINVAL

    def put(field, value, k=None):
        def change(e):
            if k is None:
                e[field] = value
            else:
                e["addr"][k][field] = value
        return change
    assert refused(put("naddr", 17)) and refused(put("naddr", 0xFFFFFFFF))
    assert refused(put("mtu", 67)) and refused(put("mtu", 0)) and not refused(put("mtu", 68))
    for af in (0, 5, 2, 10):
        assert refused(put("af", af, 3)) and refused(put("af", af, 15))
    assert refused(put("af", 6, 8))       # an af-6 entry behind the first af-4 one
    assert not refused(put("af", 6, 7))   # (the first af-4 entry itself: the boundary moves)
    assert refused(put("af", 4, 0))       # an af-4 entry in front of af-6 ones
    assert not refused(put("af", 4, 6))   # the boundary moves: still IPv6 first
    e = full.copy()
    e[0]["naddr"], e[0]["addr"][12]["af"] = 12, 9  # past naddr: not looked at
    assert lib.wc_rx_engine_check(e.ctypes.data) == OK
    wc.rx_engine_check(good)
    bad = good.copy()
    bad[0]["mtu"] = 40
    with pytest.raises(ValueError):
        wc.rx_engine_check(bad)


def plan(lib, base=P, off=P, flen=P, n=8, verdict=P, sock=None, eng=P, slot=2048, action=P,
         rlen=P, lst=None, cnt=None, scratch=None):
    return lib.wc_rx_reply_plan(base, off, flen, n, verdict, sock, eng, slot, action, rlen, lst,
                                cnt, scratch, None)


def test_plan_argument_errors_need_no_gpu():
    lib = _lib.load()
    # n = 0 without a count looks at no pointer
    assert lib.wc_rx_reply_plan(None, None, None, 0, None, None, None, 1 << 20, None, None, None,
                                None, None, None) == OK
    # the list and its count go together: checked first, for every n
    for n in (0, 8):
        assert plan(lib, n=n, lst=P, cnt=None, scratch=P) == EINVAL
        assert plan(lib, n=n, lst=None, cnt=P, scratch=P) == EINVAL
    assert plan(lib, n=(1 << 32) + 1) == EINVAL
    assert plan(lib, slot=65536) == EINVAL
    for missing in ("base", "off", "flen", "verdict", "eng", "action", "rlen"):
        assert plan(lib, **{missing: None}) == EINVAL, missing
    for e in (P + 1, P + 2, P + 3):
        assert plan(lib, eng=e) == EINVAL  # not 4-byte aligned
    assert plan(lib, lst=P, cnt=P, scratch=None) == EINVAL
    for s in (P + 1, P + 2, P + 3):
        assert plan(lib, lst=P, cnt=P, scratch=s) == EINVAL


def build(lib, base=P, off=P, flen=P, n=8, action=P, lst=P, cnt=P, eng=P, out=P, ooff=P, m=4,
          slot=2048, ipid=None, olen=P, built=P):
    return lib.wc_rx_reply_build(base, off, flen, n, action, lst, cnt, eng, out, ooff, m, slot,
                                 ipid, olen, built, None)


def test_build_argument_errors_need_no_gpu():
    lib = _lib.load()
    assert build(lib, n=(1 << 32) + 1) == EINVAL
    assert build(lib, slot=65536) == EINVAL
    assert build(lib, built=None) == EINVAL and build(lib, built=None, m=0) == EINVAL
    for missing in ("base", "off", "flen", "action", "lst", "cnt", "eng", "out", "ooff", "olen"):
        assert build(lib, **{missing: None}) == EINVAL, missing
    assert build(lib, n=0, olen=None) == EINVAL
    for e in (P + 1, P + 2, P + 3):
        assert build(lib, eng=e) == EINVAL


def test_python_wrappers_check_before_the_library():
    import torch
    cpu = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.rx_reply_plan(cpu, cpu, cpu, cpu, None, cpu, 2048)
    with pytest.raises(ValueError):
        wc.rx_reply_build(cpu, cpu, cpu, cpu, cpu, cpu, cpu, cpu, cpu, 2048)
    with pytest.raises(ValueError):
        wc.rx_engine_check(np.zeros(2, wc.RX_ENGINE))
