"""CPU tests of the RX neighbours' C ABI (wc_rx_neigh_plan, wc_rx_neigh_updates,
wc_rx_neigh_build): the names are exported through the header, the library and
the Python mirror, the codes and masks agree, the record is 24 bytes, and
every argument error returns before a device is touched (there is no GPU here;
the pointers are poisoned)."""
import re
import subprocess
from pathlib import Path

import pytest

import rx_neigh_model as model
import warpcore_amd as wc
from warpcore_amd import _build, _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
CALLS = ("wc_rx_neigh_plan", "wc_rx_neigh_updates", "wc_rx_neigh_build")


def test_neigh_names_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    for name in CALLS:
        assert f" T {name}\n" in syms
        assert name in _lib.SIGNATURES
        assert re.search(rf"\bint {name}\(", text)
    for name in ("rx_neigh_plan", "rx_neigh_updates", "rx_neigh_build", "NEIGH_UPDATE",
                 "RN_MASK_REPLY", "RN_MASK_UPDATE", "RN_NAMES"):
        assert name in wc.__all__ and hasattr(wc, name)
    for name, code in (("NONE", 0), ("MALFORMED", 4), ("UPDATE4", 8), ("ARP_IS_AT", 9),
                       ("NADV", 10), ("UPDATE6", 11)):
        assert re.search(rf"\bWC_RN_{name} = {code}\b", text)
        assert getattr(wc, f"RN_{name}") == code == getattr(model, name)
        assert f"RN_{name}" in wc.__all__ and code in wc.RN_NAMES
    assert "#define WC_RN_MASK_REPLY  (0x600u)" in text and "#define WC_RN_MASK_UPDATE (0xF00u)" in text
    assert wc.RN_MASK_REPLY == model.MASK_REPLY == sum(1 << a for a in model.REPLIES) == 0x600
    assert wc.RN_MASK_UPDATE == model.MASK_UPDATE == sum(1 << a for a in model.UPDATES) == 0xF00
    assert wc.RN_MALFORMED == wc.RR_MALFORMED and max(model.ALL_ACTIONS) < 32


def test_new_sources_are_built_and_read_no_environment():
    names = {p.name for p in _build.HIP_SOURCES}
    assert {"wc_k_rxneigh.hip", "wc_rt_rxneigh.cpp"} <= names
    assert "wc_rx_neigh.h" in {p.name for p in _build.HIP_DEPS}
    for name in ("wc_k_rxneigh.hip", "wc_rt_rxneigh.cpp", "wc_rx_neigh.h"):
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_record_size_and_layout(tmp_path):
    assert wc.NEIGH_UPDATE.itemsize == 24 and wc.NEIGH_UPDATE == model.UPDATE
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu\\n\", "
                   "sizeof(struct wc_neigh_update), offsetof(struct wc_neigh_update, af), "
                   "offsetof(struct wc_neigh_update, action), offsetof(struct wc_neigh_update, mac), "
                   "offsetof(struct wc_neigh_update, addr), sizeof(enum wc_rx_neigh_action)); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out][:5] == [24, 0, 1, 2, 8]
    f = wc.NEIGH_UPDATE.fields
    assert (f["af"][1], f["action"][1], f["mac"][1], f["addr"][1]) == (0, 1, 2, 8)


def plan(lib, base=P, off=P, flen=P, n=8, action=P, eng=P, nact=P, rl=None, rc=None, ul=None,
         uc=None, scratch=None):
    return lib.wc_rx_neigh_plan(base, off, flen, n, action, eng, nact, rl, rc, ul, uc, scratch, None)


def test_plan_argument_errors_need_no_gpu():
    lib = _lib.load()
    # n = 0 without a count looks at no pointer
    assert lib.wc_rx_neigh_plan(None, None, None, 0, None, None, None, None, None, None, None,
                                None, None) == OK
    # each list and its count go together: checked first, for every n
    for n in (0, 8, (1 << 32) + 1):
        for kw in (dict(rl=P), dict(rc=P), dict(ul=P), dict(uc=P), dict(rl=P, rc=P, ul=P),
                   dict(rl=P, ul=P, uc=P)):
            assert plan(lib, n=n, scratch=P, **kw) == EINVAL, (n, kw)
    assert plan(lib, n=(1 << 32) + 1) == EINVAL
    for missing in ("base", "off", "flen", "action", "eng", "nact"):
        assert plan(lib, **{missing: None}) == EINVAL, missing
    for e in (P + 1, P + 2, P + 3):
        assert plan(lib, eng=e) == EINVAL  # not 4-byte aligned
    for kw in (dict(rl=P, rc=P), dict(ul=P, uc=P), dict(rl=P, rc=P, ul=P, uc=P)):
        assert plan(lib, scratch=None, **kw) == EINVAL
        for s in (P + 1, P + 2, P + 3):
            assert plan(lib, scratch=s, **kw) == EINVAL


def updates(lib, base=P, off=P, flen=P, n=8, nact=P, lst=P, cnt=P, m=4, upd=P):
    return lib.wc_rx_neigh_updates(base, off, flen, n, nact, lst, cnt, m, upd, None)


def test_updates_argument_errors_need_no_gpu():
    lib = _lib.load()
    assert lib.wc_rx_neigh_updates(None, None, None, 8, None, None, None, 0, None, None) == OK
    assert updates(lib, n=(1 << 32) + 1) == EINVAL and updates(lib, n=(1 << 32) + 1, m=0) == EINVAL
    assert updates(lib, upd=None) == EINVAL and updates(lib, upd=None, n=0) == EINVAL
    for u in (P + 1, P + 2, P + 3):
        assert updates(lib, upd=u) == EINVAL
    for missing in ("base", "off", "flen", "nact", "lst", "cnt"):
        assert updates(lib, **{missing: None}) == EINVAL, missing


def build(lib, base=P, off=P, flen=P, n=8, nact=P, lst=P, cnt=P, eng=P, out=P, ooff=P, m=4,
          slot=2048, olen=P, built=P):
    return lib.wc_rx_neigh_build(base, off, flen, n, nact, lst, cnt, eng, out, ooff, m, slot, olen,
                                 built, None)


def test_build_argument_errors_need_no_gpu():
    lib = _lib.load()
    assert build(lib, n=(1 << 32) + 1) == EINVAL
    assert build(lib, slot=65536) == EINVAL
    assert build(lib, built=None) == EINVAL and build(lib, built=None, m=0) == EINVAL
    for missing in ("base", "off", "flen", "nact", "lst", "cnt", "eng", "out", "ooff", "olen"):
        assert build(lib, **{missing: None}) == EINVAL, missing
    assert build(lib, n=0, olen=None) == EINVAL
    for e in (P + 1, P + 2, P + 3):
        assert build(lib, eng=e) == EINVAL


def test_python_wrappers_check_before_the_library():
    import torch
    cpu = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.rx_neigh_plan(cpu, cpu, cpu, cpu, cpu)
    with pytest.raises(ValueError):
        wc.rx_neigh_updates(cpu, cpu, cpu, cpu, cpu, cpu, 4)
    with pytest.raises(ValueError):
        wc.rx_neigh_build(cpu, cpu, cpu, cpu, cpu, cpu, cpu, cpu, cpu, 2048)
