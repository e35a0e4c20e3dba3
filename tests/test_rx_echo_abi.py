"""CPU tests of the RX echo's C ABI (wc_rx_echo): the name is exported through
the header, the library and the Python mirror, the constants agree, struct
wc_rx_echo_out has the layout of its ctypes mirror, the new sources are built
and read no environment, and every argument error returns before a device is
touched (there is no GPU here; the pointers are poisoned and never
dereferenced)."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import warpcore_amd as wc
from warpcore_amd import _build, _lib
from warpcore_amd.cksum import _EchoOut

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
MEMBERS = [name for name, _ in _EchoOut._fields_]
RX = ("base", "off", "flen", "rec", "lst", "start", "emap")


def test_names_and_constants():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    assert " T wc_rx_echo\n" in syms
    assert re.search(r"\bint wc_rx_echo\(", text)
    for name, value, mirror in (("WC_ECHO_OFF", "0xFFFFu", wc.ECHO_OFF),
                                ("WC_RX_ECHO_MAX", "65536u", wc.RX_ECHO_MAX)):
        m = re.search(rf"#define {name}\s+(\S+)", text)
        assert m and m.group(1) == value and mirror == int(value.rstrip("u"), 0), name
    for name, value in (("ECHO", 0), ("NONE", 4), ("SHORT", 8), ("NO_ROOM", 9), ("STALE", 10)):
        assert re.search(rf"\bWC_EC_{name}\s*=\s*{value},", text), name
        assert getattr(wc, f"EC_{name}") == value and value in wc.EC_NAMES and value < 32
    assert wc.EC_MASK_SKIPPED == (1 << 8) | (1 << 9) | (1 << 10)
    # the two deliberate differences are stated
    assert "PLACEHOLDER" in text and "shifts the frame start instead" in text
    assert "reduced by the largest shift, 40" in text
    assert "wc_rx_echo" in _lib.SIGNATURES and len(_lib.SIGNATURES["wc_rx_echo"][1]) == 16
    for name in ("rx_echo", "RxEcho", "RX_ECHO_MAX", "ECHO_OFF", "EC_ECHO", "EC_NONE", "EC_SHORT",
                 "EC_NO_ROOM", "EC_STALE", "EC_NAMES"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert wc.RxEcho._fields == ("descs", "dsts", "af", "status", "src", "tx_off", "count",
                                 "skipped")


def test_new_sources_are_built_and_read_no_environment():
    assert {"wc_k_rxecho.hip", "wc_rt_rxecho.cpp"} <= {p.name for p in _build.HIP_SOURCES}
    assert "wc_rx_echo.h" in {p.name for p in _build.HIP_DEPS}
    for name in ("wc_k_rxecho.hip", "wc_rt_rxecho.cpp", "wc_rx_echo.h"):
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_struct_layout_is_the_mirrors(tmp_path):
    src = tmp_path / "sizes.c"
    offs = ", ".join(f"offsetof(struct wc_rx_echo_out, {m})" for m in MEMBERS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { size_t v[] = {sizeof(struct wc_rx_echo_out), "
                   f"{offs}}};\n"
                   "for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%zu \", v[i]); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_EchoOut)
    assert out[1:] == [getattr(_EchoOut, m).offset for m in MEMBERS]
    assert len(MEMBERS) == 8 and all(t is ctypes.c_void_p for _, t in _EchoOut._fields_)


def echo(lib, mode="copy", n=8, ns=4, m=4, slot=2048, out=True, ip_id=P, base=P, off=P, flen=P,
         rec=P, lst=P, start=P, emap=P, out_base=None, out_off=None, **members):
    """wc_rx_echo with every pointer poisoned; mode: copy / in_place give the
    three mode pointers, anything else leaves them to the keywords."""
    vals = {x: P for x in MEMBERS}
    if mode == "copy":
        out_base, out_off, vals["tx_off"] = P, P, None
    elif mode == "in_place":
        out_base, out_off = None, None
    vals.update(members)
    o = _EchoOut(*[vals[x] for x in MEMBERS])
    return lib.wc_rx_echo(base, off, flen, n, rec, lst, start, emap, ns, ip_id, out_base, out_off,
                          slot, m, ctypes.byref(o) if out else None, None)


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    for mode in ("copy", "in_place"):
        for m in (0, 1, 64, 65, 65536):
            for n, ns in ((8, 4), (0, 4), (8, 0)):
                kw = dict(mode=mode, m=m, n=n, ns=ns)
                assert echo(lib, out=False, **kw) == EINVAL
                assert echo(lib, count=None, **kw) == EINVAL
                assert echo(lib, slot=65536, **kw) == EINVAL
                for d in (1, 2, 4, 8):
                    assert echo(lib, rec=P + d, **kw) == EINVAL
            assert echo(lib, mode=mode, m=m, n=(1 << 32) + 1) == EINVAL
            assert echo(lib, mode=mode, m=m, ns=255) == EINVAL
        assert echo(lib, mode=mode, m=65537) == EINVAL
        assert echo(lib, mode=mode, m=65537, n=0) == EINVAL
        for m in (1, 64, 65536):
            for n, ns in ((8, 4), (0, 4), (8, 0)):
                kw = dict(mode=mode, m=m, n=n, ns=ns)
                for member in ("desc", "dsts", "af", "status"):
                    assert echo(lib, **{member: None}, **kw) == EINVAL, member
                for d in (1, 2, 4):
                    assert echo(lib, desc=P + d, **kw) == EINVAL
                for d in (1, 2, 3):
                    assert echo(lib, dsts=P + d, **kw) == EINVAL
            for missing in RX:  # the RX side is asked for only where there is one
                assert echo(lib, mode=mode, m=m, **{missing: None}) == EINVAL, missing
    for m in (1, 64, 65536):
        for n in (8, 0):
            kw = dict(mode=None, m=m, n=n)
            # both modes, neither mode, and the halves of one
            assert echo(lib, out_base=P, out_off=P, tx_off=P, **kw) == EINVAL
            assert echo(lib, out_base=None, out_off=None, tx_off=None, **kw) == EINVAL
            assert echo(lib, out_base=P, out_off=None, tx_off=None, **kw) == EINVAL
            assert echo(lib, out_base=None, out_off=P, tx_off=None, **kw) == EINVAL
            assert echo(lib, out_base=P, out_off=None, tx_off=P, **kw) == EINVAL
            for d in (1, 2, 4):
                assert echo(lib, out_base=P, out_off=P + d, tx_off=None, **kw) == EINVAL
                assert echo(lib, out_base=None, out_off=None, tx_off=P + d, **kw) == EINVAL


def test_a_good_call_goes_on_to_the_device():
    """Past the argument checks the call is no WC_EINVAL.  With a GPU, m = 0
    and no frame need nothing but the count, which is device memory and is
    written (everything else: test_gpu_rx_echo.py); without one the call fails
    with another code before anything is launched, and the host word it was
    handed is never reached."""
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        count = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        o = _EchoOut(None, None, None, None, None, None, count.data_ptr(), None)
        rc = lib.wc_rx_echo(None, None, None, 0, None, None, None, None, 0, None, None, None, 0, 0,
                            ctypes.byref(o), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == OK and count.item() == 0
        return
    host = (ctypes.c_uint64 * 1)(7)
    for mode in ("copy", "in_place"):
        for n, ns, m in ((8, 4, 4), (0, 0, 4), (8, 4, 0), (0, 0, 0)):
            rc = echo(lib, mode=mode, n=n, ns=ns, m=m, count=ctypes.addressof(host))
            assert rc not in (OK, EINVAL) and host[0] == 7
    none = dict(base=None, off=None, flen=None, rec=None, lst=None, start=None, emap=None)
    assert echo(lib, n=0, ns=4, count=ctypes.addressof(host), **none) not in (OK, EINVAL)
    assert echo(lib, n=8, ns=0, count=ctypes.addressof(host), **none) not in (OK, EINVAL)


def test_python_wrapper_checks_before_the_library():
    import torch
    cpu = torch.zeros(4096, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.rx_echo(cpu, cpu, cpu, (cpu, cpu, cpu), cpu, 4)
    with pytest.raises(ValueError):
        wc.rx_echo(cpu, cpu, cpu, None, cpu, 4)
