"""CPU tests of the RX answer's C ABI (wc_rx_answer_scratch, wc_rx_answer): the
names are exported through the header, the library and the Python mirror, the
constant agrees, struct wc_rx_answer_io has the layout of its ctypes mirror, the
scratch size is wc_neigh_apply's, and every argument error returns before a
device is touched (there is no GPU here; the pointers are poisoned and never
dereferenced), at list sizes on both sides of WC_RX_ANSWER_SMALL."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import warpcore_amd as wc
from warpcore_amd import _build, _lib
from warpcore_amd.cksum import _AnswerIo

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
MEMBERS = [name for name, _ in _AnswerIo._fields_]
COUNTS = ("r_m", "n_m", "u_m")
OPTIONAL = ("ip_id", "dropped", "tab")


def test_names_and_constant():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    assert " T wc_rx_answer\n" in syms and " T wc_rx_answer_scratch\n" in syms
    assert re.search(r"\bint wc_rx_answer\(", text)
    assert re.search(r"\buint64_t wc_rx_answer_scratch\(uint32_t u_m\)", text)
    m = re.search(r"#define WC_RX_ANSWER_SMALL\s+(\S+)", text)
    assert m and m.group(1) == "4096u" and wc.RX_ANSWER_SMALL == 4096
    m = re.search(r"#define WC_RX_ANSWER_SMALL_APPLY\s+(\S+)", text)
    assert m and m.group(1) == "1024u" and wc.RX_ANSWER_SMALL_APPLY == 1024
    assert "must not overlap each other" in text  # the one new precondition is stated
    for name in ("wc_rx_answer", "wc_rx_answer_scratch"):
        assert name in _lib.SIGNATURES
    for name in ("rx_answer", "rx_answer_scratch", "RxAnswer", "RX_ANSWER_SMALL"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert wc.RxAnswer._fields == ("reply_lens", "reply_built", "neigh_lens", "neigh_built",
                                   "updates", "dropped")


def test_new_sources_are_built_and_read_no_environment():
    names = {p.name for p in _build.HIP_SOURCES}
    assert {"wc_k_rxanswer.hip", "wc_rt_rxanswer.cpp"} <= names
    assert {"wc_rx_answer.h", "wc_rx_build.h"} <= {p.name for p in _build.HIP_DEPS}
    for name in ("wc_k_rxanswer.hip", "wc_rt_rxanswer.cpp", "wc_rx_answer.h", "wc_rx_build.h"):
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_scratch_size():
    lib = _lib.load()
    assert lib.wc_rx_answer_scratch(0) == 0 == wc.rx_answer_scratch(0)
    ms = sorted(set(list(range(0, 70)) + [255, 256, 257, 4095, 4096, 4097, 65535, 65536]
                    + [(1 << k) + d for k in (20, 26, 31) for d in (-1, 0, 1)] + [0xFFFFFFFF]))
    sizes = [lib.wc_rx_answer_scratch(m) for m in ms]
    for i, m in enumerate(ms):
        assert sizes[i] == lib.wc_neigh_apply_scratch(m) == wc.rx_answer_scratch(m), m
        assert i == 0 or sizes[i - 1] <= sizes[i], "never decreasing"
        assert (sizes[i] > 0) == (m > 0)


def test_struct_layout_is_the_mirrors(tmp_path):
    src = tmp_path / "sizes.c"
    offs = ", ".join(f"offsetof(struct wc_rx_answer_io, {m})" for m in MEMBERS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { size_t v[] = {sizeof(struct wc_rx_answer_io), "
                   f"{offs}}};\n"
                   "for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%zu \", v[i]); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_AnswerIo)
    assert out[1:] == [getattr(_AnswerIo, m).offset for m in MEMBERS]
    assert len(MEMBERS) == 23
    for m, t in _AnswerIo._fields_:
        assert t is (ctypes.c_uint32 if m in COUNTS else ctypes.c_void_p), m


def answer(lib, base=P, off=P, flen=P, n=8, eng=P, slot=2048, io=True, scratch=P, m=4,
           **members):
    vals = {x: (m if x in COUNTS else P) for x in MEMBERS}
    vals.update(members)
    o = _AnswerIo(*[vals[x] for x in MEMBERS])
    return lib.wc_rx_answer(base, off, flen, n, eng, slot, ctypes.byref(o) if io else None,
                            scratch, None)


SIZES = [4, 1024, 1025, 4095, 4096, 4097, 5000]  # both paths, and the apply's own threshold


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    for m in SIZES + [0]:
        for n in (8, 0):
            assert answer(lib, m=m, n=n, io=False) == EINVAL
            assert answer(lib, m=m, n=n, r_built=None) == EINVAL
            assert answer(lib, m=m, n=n, n_built=None) == EINVAL
            assert answer(lib, m=m, n=n, slot=65536) == EINVAL
        assert answer(lib, m=m, n=(1 << 32) + 1) == EINVAL
    for m in SIZES:
        # each part alone above zero, the other two empty: its own call's rules
        parts = {
            "r_m": ("action", "rlist", "rcount", "r_out_base", "r_out_off"),
            "n_m": ("nact", "nrlist", "nrcount", "n_out_base", "n_out_off"),
            "u_m": ("nact", "ulist", "ucount"),
        }
        for part, ptrs in parts.items():
            only = {c: (m if c == part else 0) for c in COUNTS}
            for missing in ("base", "off", "flen") + (("eng",) if part != "u_m" else ()):
                assert answer(lib, **only, **{missing: None}) == EINVAL, (m, part, missing)
            for missing in ptrs:
                assert answer(lib, **only, **{missing: None}) == EINVAL, (m, part, missing)
            if part != "u_m":
                for d in (1, 2, 3):
                    assert answer(lib, **only, eng=P + d) == EINVAL, (m, part, d)
        # the outputs of a part are asked for even without a frame
        assert answer(lib, m=0, r_m=m, n=0, r_out_len=None) == EINVAL
        assert answer(lib, m=0, n_m=m, n=0, n_out_len=None) == EINVAL
        assert answer(lib, m=0, u_m=m, n=0, upd=None) == EINVAL
        assert answer(lib, m=0, r_m=m, r_out_len=None) == EINVAL
        assert answer(lib, m=0, n_m=m, n_out_len=None) == EINVAL
        for d in (1, 2, 3):
            assert answer(lib, m=0, u_m=m, upd=P + d) == EINVAL
            assert answer(lib, m=0, u_m=m, n=0, upd=P + d) == EINVAL
        # with a table and u_m > 0: wc_neigh_apply's rules, with or without a frame
        for n in (8, 0):
            only = dict(m=0, u_m=m, n=n)
            assert answer(lib, **only, scratch=None) == EINVAL
            assert answer(lib, **only, ucount=None) == EINVAL
            for d in (1, 2, 3):
                assert answer(lib, **only, scratch=P + d) == EINVAL
            for d in (1, 2, 4, 8):
                assert answer(lib, **only, tab=P + d) == EINVAL
    assert answer(lib, m=0, u_m=(1 << 31) + 1, n=0) == EINVAL  # wc_neigh_apply's limit


def test_all_m_zero_needs_nothing_but_the_two_counts():
    """All three m zero with every other pointer NULL is no argument error: the
    call goes on to the device to write the two zero counts.  They are therefore
    real memory -- device memory where there is a GPU, and then the call
    succeeds and writes them; host words where there is none, and then it fails
    with another code before anything is launched."""
    import torch
    lib = _lib.load()
    none = {x: None for x in MEMBERS if x not in COUNTS}
    if torch.cuda.is_available():
        counts = torch.full((2,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        none.update(r_built=counts.data_ptr(), n_built=counts.data_ptr() + 8)
        for n in (0, 600):
            counts.fill_(0x5A5A5A5A)
            torch.cuda.synchronize()
            o = _AnswerIo(**{k: (0 if k in COUNTS else v) for k, v in
                             {**{c: 0 for c in COUNTS}, **none}.items()})
            rc = lib.wc_rx_answer(None, None, None, n, None, 0, ctypes.byref(o), None,
                                  torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == OK and counts.tolist() == [0, 0]
    else:
        host = (ctypes.c_uint64 * 2)(7, 7)
        none.update(r_built=ctypes.addressof(host), n_built=ctypes.addressof(host) + 8)
        for n in (0, 600):
            rc = answer(lib, base=None, off=None, flen=None, n=n, eng=None, scratch=None, m=0,
                        **none)
            assert rc not in (OK, EINVAL) and list(host) == [7, 7]


def test_python_wrapper_checks_before_the_library():
    import torch
    cpu = torch.zeros(64 + 32 * 64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.rx_answer(cpu, cpu, cpu, (cpu,) * 8, cpu, cpu, cpu, cpu, cpu, 4)
    with pytest.raises(ValueError):
        wc.rx_answer(cpu, cpu, cpu, None, cpu, cpu, cpu, cpu, cpu, 4)
