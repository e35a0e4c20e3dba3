"""CPU tests of the TX build's C ABI (wc_tx_socks_check, wc_tx_build_ragged,
wc_tx_build_host): the names are exported through the header, the library and
the Python mirror, the structs are 52 / 24 / 8 bytes, and every argument error
returns before a device is touched (there is no GPU here; the pointers are
poisoned)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tx_build_model as model
import warpcore_amd as wc
from warpcore_amd import _build, _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
ZERO_UDP, NO_STORE = 1, 2
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first


def test_build_names_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    for name in ("wc_tx_socks_check", "wc_tx_build_ragged", "wc_tx_build_host"):
        assert f" T {name}\n" in syms
        assert name in _lib.SIGNATURES
        assert re.search(rf"\bint {name}\(", text)
    for name in ("tx_socks_check", "tx_build_ragged", "tx_build_host", "TX_SOCK", "TX_DST",
                 "TX_DESC", "TX_SOCK_CONNECTED", "TX_SOCK_ECN"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert "#define WC_TX_BUILD_MAX_SOCKS 256" in text
    assert re.search(r"#define WC_TX_SOCK_CONNECTED 1u", text) and wc.TX_SOCK_CONNECTED == 1
    assert re.search(r"#define WC_TX_SOCK_ECN +2u", text) and wc.TX_SOCK_ECN == 2
    assert text.index("TX build") > text.index("int wc_tx_seal_host(")  # below the TX seal


def test_struct_sizes_and_layouts(tmp_path):
    assert (wc.TX_SOCK.itemsize, wc.TX_DST.itemsize, wc.TX_DESC.itemsize) == (52, 24, 8)
    assert (wc.TX_SOCK, wc.TX_DST, wc.TX_DESC) == (model.SOCK, model.DST, model.DESC)
    # the header's own structs, through a C compiler
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu\\n\", "
                   "sizeof(struct wc_tx_sock), sizeof(struct wc_tx_dst), sizeof(struct wc_tx_desc), "
                   "offsetof(struct wc_tx_sock, smac), offsetof(struct wc_tx_sock, laddr), "
                   "offsetof(struct wc_tx_sock, raddr), offsetof(struct wc_tx_dst, port), "
                   "offsetof(struct wc_tx_desc, dst)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [52, 24, 8, 6, 20, 36, 22, 6]
    assert wc.TX_SOCK.fields["smac"][1] == 6 and wc.TX_SOCK.fields["laddr"][1] == 20
    assert wc.TX_SOCK.fields["raddr"][1] == 36 and wc.TX_DST.fields["port"][1] == 22
    assert wc.TX_DESC.fields["dst"][1] == 6


def build(lib, base=P, off=P, desc=P, n=8, socks=P, ns=4, dsts=P, ndst=4, slot=2048, flags=0,
          flen=P, status=P, oip=None, oudp=None, errs=None):
    return lib.wc_tx_build_ragged(base, off, desc, n, socks, ns, dsts, ndst, slot, flags, flen,
                                  status, oip, oudp, errs, None)


def test_build_ragged_argument_errors_need_no_gpu():
    lib = _lib.load()
    # n = 0 looks at no pointer
    assert lib.wc_tx_build_ragged(None, None, None, 0, None, 999, None, 1 << 20, 0, 0xFF, None,
                                  None, None, None, None, None) == OK
    for missing in ("base", "off", "desc", "flen", "status"):
        assert build(lib, **{missing: None}) == EINVAL, missing
    assert build(lib, socks=None, ns=1) == EINVAL
    assert build(lib, dsts=None, ndst=1) == EINVAL
    assert build(lib, ns=257) == EINVAL
    assert build(lib, ndst=65537) == EINVAL
    for d in (P + 1, P + 2, P + 4):
        assert build(lib, desc=d) == EINVAL  # not 8-byte aligned
    for t in (P + 1, P + 2, P + 3):
        assert build(lib, socks=t) == EINVAL  # not 4-byte aligned
        assert build(lib, dsts=t) == EINVAL
    for flags in (4, 8, 0x80000000, ZERO_UDP | 4):
        assert build(lib, flags=flags) == EINVAL
    # compute only: both value arrays are required
    assert build(lib, flags=NO_STORE) == EINVAL
    assert build(lib, flags=NO_STORE, oip=P) == EINVAL
    assert build(lib, flags=NO_STORE | ZERO_UDP, oudp=P) == EINVAL


def test_build_host_argument_errors_need_no_gpu():
    lib = _lib.load()
    buf = np.zeros(200, dtype=np.uint8)
    off = np.array([20], dtype=np.uint64)
    desc = np.zeros(1, dtype=wc.TX_DESC)
    desc["data_len"] = 100
    socks = np.zeros(1, dtype=wc.TX_SOCK)
    socks["af"], socks["flags"] = 4, wc.TX_SOCK_CONNECTED
    flen, st = np.zeros(1, np.uint16), np.zeros(1, np.uint8)
    b, o, d, s, f, t = (a.ctypes.data for a in (buf, off, desc, socks, flen, st))

    def host(base=b, nbytes=200, offs=o, descs=d, n=1, sk=s, ns=1, ds=None, ndst=0, slot=2048,
             flags=0, fl=f, status=t, errs=None):
        return lib.wc_tx_build_host(base, nbytes, offs, descs, n, sk, ns, ds, ndst, slot, flags,
                                    fl, status, errs)

    errs = ctypes.c_uint64(7)
    assert lib.wc_tx_build_host(None, 0, None, None, 0, None, 0, None, 0, 0, 0, None, None,
                                ctypes.byref(errs)) == OK and errs.value == 0
    for missing in ("base", "offs", "descs", "fl", "status"):
        assert host(**{missing: None}) == EINVAL, missing
    assert host(sk=None) == EINVAL and host(ds=None, ndst=1) == EINVAL
    assert host(ns=257) == EINVAL and host(ds=P, ndst=65537) == EINVAL
    assert host(descs=d + 4) == EINVAL and host(sk=s + 2) == EINVAL and host(ds=P + 1, ndst=1) == EINVAL
    assert host(flags=NO_STORE) == EINVAL and host(flags=4) == EINVAL
    # the 142-byte frame must lie inside the region, before any byte is written
    off[0] = 59
    assert host() == EINVAL
    off[0] = 201
    assert host(flags=ZERO_UDP) == EINVAL
    assert not buf.any()


def test_socks_check():
    lib = _lib.load()
    socks = np.zeros(256, dtype=wc.TX_SOCK)
    socks["af"] = np.where(np.arange(256) & 1, 6, 4)
    socks["flags"] = np.arange(256) & 3
    s = socks.ctypes.data
    assert lib.wc_tx_socks_check(None, 0) == OK
    assert lib.wc_tx_socks_check(s, 256) == OK
    assert lib.wc_tx_socks_check(s, 257) == EINVAL
    assert lib.wc_tx_socks_check(None, 1) == EINVAL
    for af in (0, 5, 2, 10):
        bad = socks.copy()
        bad["af"][200] = af
        assert lib.wc_tx_socks_check(bad.ctypes.data, 256) == EINVAL
        assert lib.wc_tx_socks_check(bad.ctypes.data, 200) == OK  # the entry is not looked at
    for flags in (4, 0x80, 7):
        bad = socks.copy()
        bad["flags"][3] = flags
        assert lib.wc_tx_socks_check(bad.ctypes.data, 256) == EINVAL
    wc.tx_socks_check(socks)
    wc.tx_socks_check(socks[:0])
    bad = socks.copy()
    bad["af"][0] = 5
    with pytest.raises(ValueError):
        wc.tx_socks_check(bad)
