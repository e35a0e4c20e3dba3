"""Python mirror of warpcore's checksum interface, backed by the gfx950 library.

Names and argument meaning follow the reference
(/root/reference/lib/src/in_cksum.h:32-36):

* :func:`ip_cksum` ``(buf, len)`` -- RFC 1071 checksum of ``len`` bytes
  (in_cksum.c:133-137);
* :func:`payload_cksum` ``(buf, len)`` -- UDP/ICMPv6 checksum with the IPv4 or
  IPv6 pseudo-header, ``buf`` at the IP header and ``len`` = IP header + UDP
  length (in_cksum.c:140-167).

Both return the checksum as the native ``uint16`` the reference returns (its
in-memory bytes are the network-order checksum).  Around them sit the batch
calls the reference's per-packet loops would use at their batch points
(backend_netmap.c:348-358 TX, 379-391 RX) on device-resident ``torch``
buffers.  Every call goes through libwccksum.so; nothing here computes a
checksum on the CPU.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib

KIND_IP = 0
KIND_PAYLOAD = 1
_KINDS = {"ip": KIND_IP, "payload": KIND_PAYLOAD, KIND_IP: KIND_IP,
          KIND_PAYLOAD: KIND_PAYLOAD}


_WC_EINVAL = -10001  # WC_EINVAL (include/warpcore_gpu/wc_cksum.h)


class WcError(RuntimeError):
    """A libwccksum call returned an error code."""

    def __init__(self, func: str, code: int):
        msg = _lib.active().wc_strerror(code).decode()
        super().__init__(f"{func}: {msg} ({code})")
        self.code = code


def _check(func: str, rc: int) -> None:
    if rc != 0:
        raise WcError(func, rc)


def _kind(kind) -> int:
    try:
        return _KINDS[kind]
    except KeyError:
        raise ValueError(f"kind must be 'ip' or 'payload', not {kind!r}") from None


def _stream_ptr(stream, device=None) -> int:
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    if isinstance(stream, torch.cuda.Stream):
        return stream.cuda_stream
    return int(stream)


def _dev_ptr(t: Union[torch.Tensor, int]) -> int:
    if isinstance(t, torch.Tensor):
        if not t.is_cuda:
            raise ValueError("batch buffers must be device (cuda) tensors")
        return t.data_ptr()
    return int(t)


def reload_config() -> None:
    """Re-read the WC_* environment (read once at first init).  The shipped
    library reads only the server's knobs (_lib.INTEGRATOR_KNOBS); while any
    path knob (WC_SHAPE, WC_SEG, WC_RX_EARLY, ...) is set, the calls of this
    module go to the tuning build, which reads them (tools and the tests that
    pin every path against the oracle)."""
    _check("wc_config_reload", _lib.select_for_env().wc_config_reload())


def _span(length: int, kind: int) -> int:
    # payload_cksum reads the IPv4 header fields up to byte 19 whatever len is
    # (in_cksum.c:149-151)
    return max(length, 20) if kind == KIND_PAYLOAD else length


def _check_len(length: int) -> int:
    if not 0 <= int(length) <= 0xFFFF:
        raise ValueError("len is a uint16 in the reference (0..65535)")
    return int(length)


def _same_device(base: torch.Tensor, **others) -> None:
    if not isinstance(base, torch.Tensor) or not base.is_cuda:
        raise ValueError("base must be a device (cuda) tensor")
    for name, t in others.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a device (cuda) tensor")
        if t.device != base.device:
            raise ValueError(f"{name} is on {t.device}, base on {base.device}")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _check_strided(base: torch.Tensor, byte_offset: int, stride: int, length: int, n: int,
                   kind: int) -> None:
    if byte_offset < 0 or stride < 0 or n < 0:
        raise ValueError("byte_offset, stride and n must be >= 0")
    if not base.is_contiguous():
        raise ValueError("base must be contiguous")
    if n and byte_offset + (n - 1) * stride + _span(length, kind) > _nbytes(base):
        raise ValueError(f"batch of {n} x {length} B at stride {stride} (+{byte_offset}) "
                         f"runs past the {_nbytes(base)}-byte buffer")


def _ip4_hl(first: torch.Tensor) -> torch.Tensor:
    """4 * IHL of the packets whose first byte says IPv4, else 0 (int64)."""
    b = first.to(torch.int64)
    return torch.where(b >> 4 == 4, (b & 0x0F) * 4, torch.zeros_like(b))


def _check_strided_headers(base: torch.Tensor, byte_offset: int, stride: int, length: int,
                           n: int) -> None:
    """The fused call reads every IPv4 header whole (hl bytes, options
    included) even where len is shorter: it must lie inside base.  Only a
    packet that starts in the buffer's last 60 bytes can fail that, so only
    those first bytes are looked at (nothing is, from len 60 on)."""
    if n == 0 or length >= 60:
        return
    nbytes = _nbytes(base)
    room = nbytes - 60 - byte_offset  # a packet starting at or below it is safe
    lo = 0 if room < 0 or stride == 0 else min(n, room // stride + 1)
    hi = 1 if stride == 0 else n
    if lo >= hi:
        return
    start = byte_offset + torch.arange(lo, hi, dtype=torch.int64, device=base.device) * stride
    hl = _ip4_hl(base.view(torch.uint8).reshape(-1)[start])
    if bool((start + hl > nbytes).any()):
        raise ValueError("an IPv4 header (hl bytes, options included) runs past the buffer: it "
                         "must lie inside it even where len is shorter")


def _check_ragged(base: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
                  kind: int, check: bool, fused: bool = False, in_place: bool = False,
                  indexed: bool = False) -> int:
    """The argument rules of every packet / frame batch call; returns n.
    ``fused``: the IPv4 headers are checked too; ``in_place``: the call writes
    into ``base``; ``indexed``: a uint32 list may name the frames."""
    _same_device(base, offsets=offsets, lengths=lengths)
    n = _check_ragged_shapes(offsets, lengths)
    if not base.is_contiguous():
        raise ValueError("base must be contiguous")
    if in_place and base.element_size() != 1:
        raise ValueError("base must be a 1-byte tensor (the frames are written in place)")
    if check and n:
        # one device reduction + sync -- pass check=False on a hot loop whose
        # layout was validated once
        _ragged_bounds(_nbytes(base), offsets, lengths, kind, base if fused else None)
    if indexed and n > _RX_SELECT_MAX:
        raise ValueError("at most 2^32 frames (the indices are uint32)")
    return n


def _check_ragged_shapes(offsets: torch.Tensor, lengths: torch.Tensor) -> int:
    n = offsets.numel()
    if (lengths.numel() != n or offsets.element_size() != 8 or lengths.element_size() != 2
            or offsets.is_floating_point() or lengths.is_floating_point()):
        raise ValueError("offsets must be 8-byte and lengths 2-byte integers, same count")
    if not (offsets.is_contiguous() and lengths.is_contiguous()):
        raise ValueError("offsets and lengths must be contiguous")
    return n


def _ragged_bounds(nbytes: int, offsets: torch.Tensor, lengths: torch.Tensor,
                   kind: int, headers_of: Optional[torch.Tensor] = None) -> None:
    """Every packet (and payload_cksum's 20 header bytes) inside [0, nbytes).
    ``headers_of`` (the fused call: its base): every IPv4 header too, hl
    bytes with the options, even where len is shorter."""
    off = offsets.view(torch.int64)
    ln = lengths.view(torch.int16).to(torch.int64) & 0xFFFF
    if kind == KIND_PAYLOAD:
        ln = torch.clamp(ln, min=20)
    if bool((off < 0).any()) or int((off + ln).max()) > nbytes:
        raise ValueError("a packet [off, off + len) runs past the buffer")
    if headers_of is not None:
        hl = _ip4_hl(headers_of.view(torch.uint8).reshape(-1)[off])
        if int((off + hl).max()) > nbytes:
            raise ValueError("an IPv4 header (hl bytes, options included) runs past the buffer: "
                             "it must lie inside it even where len is shorter")


class _on_device:
    """Make base's device current for the library call (it resolves its
    device with hipGetDevice)."""

    def __init__(self, device: torch.device):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


# --------------------------------------------------------------------------
# Scalar drop-ins (reference in_cksum.h:32-36).

def _host_buffer(buf, length: Optional[int]) -> Tuple[ctypes.c_void_p, int, object]:
    arr = np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8) \
        if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    if length is None:
        length = arr.size
    if not 0 <= length <= 0xFFFF:
        raise ValueError("len is a uint16 in the reference (0..65535)")
    keep = np.ascontiguousarray(arr)
    return ctypes.c_void_p(keep.ctypes.data), length, keep


def ip_cksum(buf, length: Optional[int] = None) -> int:
    """GPU-computed ``ip_cksum(buf, len)`` (in_cksum.c:133-137)."""
    p, n, keep = _host_buffer(buf, length)
    if keep.size < n:
        raise ValueError("buffer shorter than len")
    return int(_lib.active().ip_cksum(p, n))


def payload_cksum(buf, length: Optional[int] = None) -> int:
    """GPU-computed ``payload_cksum(buf, len)`` (in_cksum.c:140-167)."""
    p, n, keep = _host_buffer(buf, length)
    if keep.size < max(n, 20):
        raise ValueError("payload_cksum reads at least the 20-byte IPv4 header")
    return int(_lib.active().payload_cksum(p, n))


# --------------------------------------------------------------------------
# Device-resident batches.

def _out_tensor(out: Optional[torch.Tensor], n: int, device) -> torch.Tensor:
    if out is None:
        out = torch.empty(n, dtype=torch.uint16, device=device)
    if out.numel() < n or out.element_size() != 2 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 2-byte tensor of >= n entries")
    if not out.is_cuda or out.device != torch.device(device):
        raise ValueError(f"out must be on {device}")
    return out


def cksum_strided(base: torch.Tensor, stride: int, length: int, n: int,
                  out: Optional[torch.Tensor] = None, kind="ip",
                  stream=None, byte_offset: int = 0) -> torch.Tensor:
    """Checksum packets ``base[byte_offset + i*stride : ... + length]``, i < n."""
    k = _kind(kind)
    _same_device(base)
    _check_strided(base, byte_offset, stride, _check_len(length), n, k)
    out = _out_tensor(out, n, base.device)
    with _on_device(base.device):
        _check("wc_cksum_strided", _lib.active().wc_cksum_strided(
            _dev_ptr(base) + byte_offset, stride, length, n, out.data_ptr(),
            k, _stream_ptr(stream, base.device)))
    return out


def cksum_ragged(base: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
                 out: Optional[torch.Tensor] = None, kind="ip",
                 stream=None, check: bool = True) -> torch.Tensor:
    """Checksum packets ``base[off[i] : off[i] + len[i]]`` (uint64 / uint16
    arrays).  ``check`` validates every packet against ``base`` (one device
    reduction and a sync); pass False on a loop over an already-checked
    layout."""
    k = _kind(kind)
    n = _check_ragged(base, offsets, lengths, k, check)
    out = _out_tensor(out, n, base.device)
    with _on_device(base.device):
        _check("wc_cksum_ragged", _lib.active().wc_cksum_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(lengths), n, out.data_ptr(),
            k, _stream_ptr(stream, base.device)))
    return out


def _bad_counter(t: Optional[torch.Tensor], device, name: str = "bad") -> torch.Tensor:
    """The counter argument ``name`` of a call that accumulates into it, or a
    zeroed one of this module's."""
    if t is None:
        return torch.zeros(1, dtype=torch.int64, device=device)
    if (t.numel() < 1 or t.dtype not in (torch.int64, torch.uint64)
            or not t.is_contiguous() or t.device != device):
        raise ValueError(f"{name} must be a contiguous int64 / uint64 device tensor (accumulated)")
    return t


def verify_strided(base, stride, length, n, kind="payload", out=None,
                   stream=None, byte_offset: int = 0,
                   bad: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """RX check (udp.c:132-139): results plus the count of non-zero checksums.
    A given ``bad`` tensor is accumulated into, not reset."""
    k = _kind(kind)
    _same_device(base)
    _check_strided(base, byte_offset, stride, _check_len(length), n, k)
    out = _out_tensor(out, n, base.device)
    bad = _bad_counter(bad, base.device)
    with _on_device(base.device):
        _check("wc_verify_strided", _lib.active().wc_verify_strided(
            _dev_ptr(base) + byte_offset, stride, length, n, out.data_ptr(), bad.data_ptr(),
            k, _stream_ptr(stream, base.device)))
    return out, bad


def verify_ragged(base, offsets, lengths, kind="payload", out=None,
                  stream=None, check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    k = _kind(kind)
    n = _check_ragged(base, offsets, lengths, k, check)
    out = _out_tensor(out, n, base.device)
    bad = torch.zeros(1, dtype=torch.int64, device=base.device)
    with _on_device(base.device):
        _check("wc_verify_ragged", _lib.active().wc_verify_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(lengths), n, out.data_ptr(),
            bad.data_ptr(), k, _stream_ptr(stream, base.device)))
    return out, bad


def cksum_ip_udp_strided(base: torch.Tensor, stride: int, length: int, n: int,
                         stream=None, byte_offset: int = 0, out_hdr: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pass over IP/UDP packets: (IPv4 header checksums, payload_cksum).
    The header checksum is ip_cksum(ip, ip4_hl) (ip4.c:110-115, 184-186); 0
    for IPv6 packets."""
    _same_device(base)
    _check_strided(base, byte_offset, stride, _check_len(length), n, KIND_PAYLOAD)
    _check_strided_headers(base, byte_offset, stride, length, n)
    hdr = _out_tensor(out_hdr, n, base.device)
    pay = _out_tensor(out, n, base.device)
    with _on_device(base.device):
        _check("wc_cksum_ip_udp_strided", _lib.active().wc_cksum_ip_udp_strided(
            _dev_ptr(base) + byte_offset, stride, length, n, hdr.data_ptr(), pay.data_ptr(),
            _stream_ptr(stream, base.device)))
    return hdr, pay


def cksum_ip_udp_ragged(base: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
                        stream=None, check: bool = True, out_hdr: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    n = _check_ragged(base, offsets, lengths, KIND_PAYLOAD, check, fused=True)
    hdr = _out_tensor(out_hdr, n, base.device)
    pay = _out_tensor(out, n, base.device)
    with _on_device(base.device):
        _check("wc_cksum_ip_udp_ragged", _lib.active().wc_cksum_ip_udp_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(lengths), n, hdr.data_ptr(),
            pay.data_ptr(), _stream_ptr(stream, base.device)))
    return hdr, pay


# --------------------------------------------------------------------------
# RX verdicts (the reference's eth_rx -> ip4_rx / ip6_rx -> udp_rx checks).

# enum wc_rx_verdict (include/warpcore_gpu/wc_cksum.h)
RX_OK, RX_OK_NO_CKSUM, RX_BAD_IP_CKSUM, RX_BAD_UDP_CKSUM, RX_SHORT, RX_FRAGMENT, \
    RX_BAD_VERSION, RX_NOT_UDP, RX_NOT_IP, RX_TRUNCATED = range(10)
RX_NAMES = ("ok", "ok_no_cksum", "bad_ip_cksum", "bad_udp_cksum", "short", "fragment",
            "bad_version", "not_udp", "not_ip", "truncated")
RX_DROPS = (RX_BAD_IP_CKSUM, RX_BAD_UDP_CKSUM, RX_SHORT, RX_FRAGMENT, RX_BAD_VERSION,
            RX_TRUNCATED)


def rx_verdict_ragged(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                      out: Optional[torch.Tensor] = None, stream=None,
                      check: bool = True,
                      drops: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """RX verdict of every Ethernet frame ``base[off[i] : off[i] + frame_len[i]]``
    (a netmap RX ring's slot buffers and slot lengths): a uint8 code per frame
    (``RX_*``) and the number of frames the reference's RX path drops.  No
    header is parsed on the host (wc_rx_verdict_ragged).  A given ``drops``
    tensor is accumulated into, not reset."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=base.device)
    if out.numel() < n or out.element_size() != 1 or not out.is_contiguous() \
            or out.device != base.device:
        raise ValueError(f"out must be a contiguous 1-byte tensor of >= n entries on {base.device}")
    drops = _bad_counter(drops, base.device, "drops")
    with _on_device(base.device):
        _check("wc_rx_verdict_ragged", _lib.active().wc_rx_verdict_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, out.data_ptr(),
            drops.data_ptr(), _stream_ptr(stream, base.device)))
    return out, drops


def rx_verdict_host(buf: np.ndarray, offsets: np.ndarray,
                    frame_lens: np.ndarray) -> Tuple[np.ndarray, int]:
    """rx_verdict_ragged over host memory (wc_rx_verdict_host, synchronous):
    (uint8 verdicts, drop count)."""
    buf, off, lens = _host_batch_args(buf, offsets, frame_lens)
    out = np.empty(off.size, dtype=np.uint8)
    drops = ctypes.c_uint64()
    _check("wc_rx_verdict_host", _lib.active().wc_rx_verdict_host(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, off.size,
        out.ctypes.data, ctypes.byref(drops)))
    return out, int(drops.value)


# --------------------------------------------------------------------------
# RX delivery (what udp_rx puts into the w_iov, and which frames to walk).

# struct wc_rx_record (include/warpcore_gpu/wc_cksum.h): 16 bytes, little-endian
RX_RECORD = np.dtype([("data_off", "<u2"), ("data_len", "<u2"), ("sport", "<u2"),
                      ("dport", "<u2"), ("af", "u1"), ("tos", "u1"), ("ttl", "u1"),
                      ("hl", "u1"), ("src_off", "<u2"), ("dst_off", "<u2")])
assert RX_RECORD.itemsize == 16
RX_MASK_DELIVER = (1 << RX_OK) | (1 << RX_OK_NO_CKSUM)
RX_MASK_HOST = (1 << RX_NOT_UDP) | (1 << RX_NOT_IP)
_RX_SELECT_MAX = 1 << 32


def rx_select_scratch(n: int) -> int:
    """Bytes of device scratch wc_rx_select needs for n frames (no GPU)."""
    return int(_lib.active().wc_rx_select_scratch(int(n)))


def _scratch(nbytes: int, device) -> torch.Tensor:
    # int32 elements: a torch allocation is aligned far beyond the 4 bytes asked
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.int32, device=device)


def _select_scratch(scratch: Optional[torch.Tensor], n: int, device) -> torch.Tensor:
    """A plan call's rx_select scratch: the caller's, checked, or one allocated here."""
    if scratch is None:
        return _scratch(rx_select_scratch(n), device)
    if _nbytes(scratch) < rx_select_scratch(n) or scratch.device != device:
        raise ValueError(f"scratch must hold rx_select_scratch(n) bytes on {device}")
    return scratch


def _index_list(out_list: Optional[torch.Tensor], n: int, device) -> Tuple[torch.Tensor, bool]:
    """The uint32 list handed to the library -- ``out_list`` or one of this
    module's -- and whether it is this module's.  It is never empty (an empty
    tensor, a zero-length slice included, has a NULL data pointer, which would
    read as "no list"); an own one is cut to n entries where it is returned."""
    own = out_list is None
    lst = torch.empty(max(n, 1), dtype=torch.uint32, device=device) if own else out_list
    if lst.numel() < max(n, 1) or lst.element_size() != 4 or not lst.is_contiguous() \
            or lst.device != device:
        raise ValueError(f"out_list must be a contiguous 4-byte tensor of >= max(n, 1) "
                         f"entries on {device}")
    return lst, own


def rx_select(verdicts: torch.Tensor, mask: int, out: Optional[torch.Tensor] = None,
              stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ascending indices i with ``(mask >> verdicts[i]) & 1`` (wc_rx_select;
    ``RX_MASK_DELIVER``, ``RX_MASK_HOST`` or any set of ``1 << RX_*``): a
    uint32 device list of ``verdicts.numel()`` entries whose first ``count``
    are written -- the rest keep what they held -- and ``count`` as a 1-element
    int64 device tensor.  Asynchronous; the scratch is allocated here."""
    _same_device(verdicts)
    if verdicts.element_size() != 1 or not verdicts.is_contiguous():
        raise ValueError("verdicts must be a contiguous 1-byte device tensor")
    n = verdicts.numel()
    if n > _RX_SELECT_MAX:
        raise ValueError("at most 2^32 frames (the indices are uint32)")
    if not 0 <= int(mask) <= 0xFFFFFFFF:
        raise ValueError("mask is a uint32 of 1 << RX_* bits")
    if out is None:
        out = torch.empty(n, dtype=torch.uint32, device=verdicts.device)
    if out.numel() < n or out.element_size() != 4 or not out.is_contiguous() \
            or out.device != verdicts.device:
        raise ValueError(f"out must be a contiguous 4-byte tensor of >= n entries on "
                         f"{verdicts.device}")
    count = torch.zeros(1, dtype=torch.int64, device=verdicts.device)
    scratch = _scratch(rx_select_scratch(n), verdicts.device)
    with _on_device(verdicts.device):
        _check("wc_rx_select", _lib.active().wc_rx_select(
            verdicts.data_ptr(), n, int(mask), out.data_ptr(), count.data_ptr(),
            scratch.data_ptr(), _stream_ptr(stream, verdicts.device)))
    return out, count


def rx_deliver_ragged(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                      want_list: bool = True, stream=None, check: bool = True,
                      out_list: Optional[torch.Tensor] = None):
    """rx_verdict_ragged plus delivery (wc_rx_deliver_ragged): returns
    ``(verdicts uint8, records, list, count, drops)`` -- ``records`` an
    ``(n, 16)`` uint8 device tensor, one struct wc_rx_record per frame (on the
    host: ``records.cpu().numpy().view(RX_RECORD)``), all-zero unless the
    verdict is RX_OK / RX_OK_NO_CKSUM; ``list`` / ``count`` as rx_select gives
    them for ``RX_MASK_DELIVER`` (None, None with ``want_list=False``);
    ``drops`` as rx_verdict_ragged.  No header is parsed on the host."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    verdicts = torch.empty(n, dtype=torch.uint8, device=d)
    records = torch.empty((n, RX_RECORD.itemsize), dtype=torch.uint8, device=d)
    drops = torch.zeros(1, dtype=torch.int64, device=d)
    lst = cnt = scratch = None
    if want_list:
        lst, own = _index_list(out_list, n, d)
        cnt = torch.zeros(1, dtype=torch.int64, device=d)
        scratch = _scratch(rx_select_scratch(n), d)
    with _on_device(d):
        _check("wc_rx_deliver_ragged", _lib.active().wc_rx_deliver_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, verdicts.data_ptr(),
            records.data_ptr(), lst.data_ptr() if want_list else None,
            cnt.data_ptr() if want_list else None, drops.data_ptr(),
            scratch.data_ptr() if want_list else None, _stream_ptr(stream, d)))
    if want_list and own:
        lst = lst[:n]
    return verdicts, records, lst, cnt, drops


def rx_deliver_host(buf: np.ndarray, offsets: np.ndarray, frame_lens: np.ndarray):
    """rx_deliver_ragged over host memory (wc_rx_deliver_host, synchronous):
    ``(uint8 verdicts, RX_RECORD records, uint32 delivered-frame indices,
    drop count)``."""
    buf, off, lens = _host_batch_args(buf, offsets, frame_lens)
    n = off.size
    verdicts = np.empty(n, dtype=np.uint8)
    records = np.zeros(n, dtype=RX_RECORD)
    lst = np.empty(max(n, 1), dtype=np.uint32)  # (never empty: its pointer must not be NULL)
    count, drops = ctypes.c_uint64(), ctypes.c_uint64()
    _check("wc_rx_deliver_host", _lib.active().wc_rx_deliver_host(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, n, verdicts.ctypes.data,
        records.ctypes.data, lst.ctypes.data, ctypes.byref(count), ctypes.byref(drops)))
    return verdicts, records, lst[:int(count.value)].copy(), int(drops.value)


# --------------------------------------------------------------------------
# RX socket demultiplex (udp_rx's w_get_sock calls and per-socket queues).

# struct wc_rx_sock (include/warpcore_gpu/wc_cksum.h): 40 bytes
RX_SOCK = np.dtype([("af", "u1"), ("connected", "u1"), ("lport", "<u2"), ("rport", "<u2"),
                    ("pad", "<u2"), ("laddr", "u1", 16), ("raddr", "u1", 16)])
assert RX_SOCK.itemsize == 40
RX_DEMUX_MAX_SOCKS = 254
RX_SOCK_NONE, RX_SOCK_UNBOUND = 0xFE, 0xFF
_RX_STARTS = 256


def rx_socktab_bytes(ns: int) -> int:
    """Bytes of the socket table of ``ns`` sockets (no GPU)."""
    return int(_lib.active().wc_rx_socktab_bytes(int(ns)))


def rx_socktab_build(socks: np.ndarray) -> np.ndarray:
    """The socket table of ``socks`` (an ``RX_SOCK`` array, at most 254
    entries; ports as the UDP header stores them) as wc_rx_socktab_build writes
    it: a uint8 array to copy to the device for rx_demux or to hand to
    rx_demux_host.  Pure host arithmetic.  ``ValueError`` for what the library
    refuses: a bad af / connected field or the same tuple twice."""
    socks = np.ascontiguousarray(socks, dtype=RX_SOCK).reshape(-1)
    ns = socks.size
    if ns > RX_DEMUX_MAX_SOCKS:
        raise ValueError(f"at most {RX_DEMUX_MAX_SOCKS} sockets (the ids are uint8)")
    tab = np.zeros(rx_socktab_bytes(ns) // 4, dtype=np.uint32)
    rc = _lib.active().wc_rx_socktab_build(socks.ctypes.data if ns else None, ns, tab.ctypes.data)
    if rc == _WC_EINVAL:
        raise ValueError("socket table: af must be 4 or 6, connected 0 or 1, every tuple distinct")
    _check("wc_rx_socktab_build", rc)
    return tab.view(np.uint8)


def _addr_bytes(af: int, addr) -> np.ndarray:
    a = np.zeros(16, dtype=np.uint8)
    b = np.frombuffer(bytes(addr), dtype=np.uint8)
    if b.size < (4 if af == 4 else 16):
        raise ValueError("an IPv4 address is 4 bytes, an IPv6 address 16")
    a[:min(b.size, 16)] = b[:16]
    return a


def rx_socktab_lookup(tab: np.ndarray, af: int, laddr, lport: int, raddr, rport: int) -> int:
    """The table's own lookup on the host (wc_rx_socktab_lookup): the connected
    tuple first, then the bound one; the socket's index or RX_SOCK_UNBOUND."""
    tab = np.ascontiguousarray(tab).view(np.uint8)
    la, ra = _addr_bytes(af, laddr), _addr_bytes(af, raddr)
    return int(_lib.active().wc_rx_socktab_lookup(tab.ctypes.data, int(af), la.ctypes.data,
                                                  int(lport), ra.ctypes.data, int(rport)))


def rx_demux_scratch(n: int) -> int:
    """Bytes of device scratch wc_rx_demux needs for n frames (no GPU)."""
    return int(_lib.active().wc_rx_demux_scratch(int(n)))


def rx_demux(base: torch.Tensor, offsets: torch.Tensor, records: torch.Tensor,
             table: torch.Tensor, ns: int, want_list: bool = True, stream=None,
             out_list: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """The socket of every delivered frame and the per-socket index lists
    (wc_rx_demux), behind an rx_deliver_ragged of the same frames whose
    ``records`` it reads; ``table``: rx_socktab_build's bytes for ``ns``
    sockets as a device tensor.  Returns ``(sock uint8, list, start)``: socket
    ``s``'s frames are ``list[start[s]:start[s + 1]]`` for ``s < 254``, the
    unbound ones ``list[start[254]:start[255]]``, ``start`` a 256-entry int64
    device tensor (None, None with ``want_list=False``).  Asynchronous; the
    scratch is allocated here unless given -- give one per call in flight when
    ``stream`` is not the current stream, so that it outlives the launches."""
    _same_device(base, offsets=offsets, records=records, table=table)
    n = offsets.numel()
    if n > _RX_SELECT_MAX:
        raise ValueError("at most 2^32 frames (the indices are uint32)")
    if offsets.element_size() != 8 or not offsets.is_contiguous() or not base.is_contiguous():
        raise ValueError("offsets must be contiguous 8-byte integers, base contiguous")
    if _nbytes(records) != n * RX_RECORD.itemsize or not records.is_contiguous():
        raise ValueError("records must be the contiguous (n, 16) bytes of rx_deliver_ragged")
    if not 0 <= int(ns) <= RX_DEMUX_MAX_SOCKS:
        raise ValueError(f"ns must be 0..{RX_DEMUX_MAX_SOCKS}")
    if not table.is_contiguous() or _nbytes(table) < rx_socktab_bytes(ns):
        raise ValueError("table must hold the rx_socktab_build bytes of ns sockets")
    d = base.device
    sock = torch.empty(n, dtype=torch.uint8, device=d)
    lst = start = None
    if want_list:
        lst, own = _index_list(out_list, n, d)
        start = torch.zeros(_RX_STARTS, dtype=torch.int64, device=d)
        if scratch is None:
            scratch = _scratch(rx_demux_scratch(n), d)
        elif _nbytes(scratch) < rx_demux_scratch(n) or scratch.device != d:
            raise ValueError(f"scratch must hold rx_demux_scratch(n) bytes on {d}")
    with _on_device(d):
        _check("wc_rx_demux", _lib.active().wc_rx_demux(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(records), n, _dev_ptr(table), int(ns),
            sock.data_ptr() if n else None, lst.data_ptr() if want_list else None,
            start.data_ptr() if want_list else None,
            scratch.data_ptr() if want_list else None, _stream_ptr(stream, d)))
    if want_list and own:
        lst = lst[:n]
    return sock, lst, start


def rx_demux_host(buf: np.ndarray, offsets: np.ndarray, frame_lens: np.ndarray,
                  tab: np.ndarray, ns: int):
    """rx_deliver_host plus the demultiplex (wc_rx_demux_host, synchronous):
    ``(uint8 verdicts, RX_RECORD records, uint8 socket ids, uint32 list,
    uint64 start[256], drop count)``; ``tab``: rx_socktab_build's bytes for
    ``ns`` sockets."""
    buf, off, lens = _host_batch_args(buf, offsets, frame_lens)
    n = off.size
    tab = np.ascontiguousarray(tab).view(np.uint8)
    if tab.size < rx_socktab_bytes(ns) or tab.ctypes.data % 4:
        raise ValueError("tab must hold the 4-byte-aligned rx_socktab_build bytes of ns sockets")
    verdicts = np.empty(n, dtype=np.uint8)
    records = np.zeros(n, dtype=RX_RECORD)
    sock = np.empty(n, dtype=np.uint8)
    lst = np.empty(max(n, 1), dtype=np.uint32)  # (never empty: its pointer must not be NULL)
    start = np.empty(_RX_STARTS, dtype=np.uint64)
    drops = ctypes.c_uint64()
    _check("wc_rx_demux_host", _lib.active().wc_rx_demux_host(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, n, tab.ctypes.data, int(ns),
        verdicts.ctypes.data, records.ctypes.data, sock.ctypes.data, lst.ctypes.data,
        start.ctypes.data, ctypes.byref(drops)))
    return verdicts, records, sock, lst[:int(start[-1])].copy(), start, int(drops.value)


# --------------------------------------------------------------------------
# RX replies (the filters, the ICMP checksum verdict, echo and unreachable
# frames of eth_rx ... udp_rx / icmp*_rx).

# struct wc_rx_ifaddr / wc_rx_engine (include/warpcore_gpu/wc_cksum.h)
RX_MAX_IFADDR = 16
RX_IFADDR = np.dtype([("af", "u1"), ("pad", "u1", 3), ("addr", "u1", 16), ("bcast", "u1", 16),
                      ("snma", "u1", 16)])
RX_ENGINE = np.dtype([("mac", "u1", 6), ("mtu", "<u2"), ("naddr", "<u4"),
                      ("addr", RX_IFADDR, RX_MAX_IFADDR)])
assert (RX_IFADDR.itemsize, RX_ENGINE.itemsize) == (52, 844)
# enum wc_rx_reply_action
RR_NONE, RR_HOST, RR_FILTERED, RR_ICMP_BAD_CKSUM, RR_MALFORMED, RR_NO_ROOM = range(6)
RR_ECHO4, RR_ECHO6, RR_UNREACH_PORT4, RR_UNREACH_PORT6, RR_UNREACH_PROTO4 = range(8, 13)
RR_MASK_REPLY = 0x1F00
RR_NAMES = {RR_NONE: "none", RR_HOST: "host", RR_FILTERED: "filtered",
            RR_ICMP_BAD_CKSUM: "icmp_bad_cksum", RR_MALFORMED: "malformed", RR_NO_ROOM: "no_room",
            RR_ECHO4: "echo4", RR_ECHO6: "echo6", RR_UNREACH_PORT4: "unreach_port4",
            RR_UNREACH_PORT6: "unreach_port6", RR_UNREACH_PROTO4: "unreach_proto4"}


def rx_engine_check(engine: np.ndarray) -> None:
    """``ValueError`` for an engine table wc_rx_engine_check refuses: more
    than 16 addresses, an af other than 4 / 6, an IPv6 entry behind an IPv4
    one, an MTU below 68.  No GPU."""
    e = np.ascontiguousarray(engine, dtype=RX_ENGINE).reshape(-1)
    if e.size != 1:
        raise ValueError("one RX_ENGINE record")
    rc = _lib.active().wc_rx_engine_check(e.ctypes.data)
    if rc == _WC_EINVAL:
        raise ValueError(f"RX engine table: at most {RX_MAX_IFADDR} addresses, af 4 or 6, the "
                         "IPv6 entries first, mtu >= 68")
    _check("wc_rx_engine_check", rc)


def _engine_tensor(engine: torch.Tensor, device) -> None:
    if not isinstance(engine, torch.Tensor) or not engine.is_cuda or engine.device != device:
        raise ValueError(f"engine must be a device tensor on {device}")
    if not engine.is_contiguous() or _nbytes(engine) != RX_ENGINE.itemsize:
        raise ValueError(f"engine must be the contiguous {RX_ENGINE.itemsize} bytes of one RX_ENGINE")


def _byte_array(name: str, t: torch.Tensor, n: int, device, size: int = 1) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise ValueError(f"{name} must be a device tensor on {device}")
    if t.element_size() != size or t.numel() < n or not t.is_contiguous() \
            or t.is_floating_point():
        raise ValueError(f"{name} must be a contiguous {size}-byte integer tensor of >= {n} entries")


def rx_reply_plan(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                  verdicts: torch.Tensor, sock: Optional[torch.Tensor], engine: torch.Tensor,
                  slot_bytes: int, want_list: bool = True, stream=None, check: bool = True,
                  out_list: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None):
    """What the reference's RX path does with every frame beyond delivering it
    (wc_rx_reply_plan), behind an rx_verdict_ragged / rx_deliver_ragged (and
    rx_demux) of the same frames whose ``verdicts`` and ``sock`` (may be None)
    it reads.  ``engine``: a device tensor holding the bytes of one
    ``RX_ENGINE`` record.  Returns ``(actions uint8 RR_*, reply_lens uint16,
    list, count)``: ``list`` / ``count`` as rx_select gives them for
    ``RR_MASK_REPLY`` (None, None with ``want_list=False``).  Asynchronous;
    the scratch is allocated here unless given."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    _byte_array("verdicts", verdicts, n, d)
    if sock is not None:
        _byte_array("sock", sock, n, d)
    _engine_tensor(engine, d)
    if not 0 <= int(slot_bytes) <= 0xFFFF:
        raise ValueError("slot_bytes is at most 65535 (a frame length is a uint16)")
    actions = torch.empty(n, dtype=torch.uint8, device=d)
    reply_lens = torch.empty(n, dtype=torch.uint16, device=d)
    lst = cnt = None
    if want_list:
        lst, own = _index_list(out_list, n, d)
        cnt = torch.zeros(1, dtype=torch.int64, device=d)
        scratch = _select_scratch(scratch, n, d)
    with _on_device(d):
        _check("wc_rx_reply_plan", _lib.active().wc_rx_reply_plan(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(verdicts),
            sock.data_ptr() if sock is not None and n else None, engine.data_ptr(),
            int(slot_bytes), actions.data_ptr() if n else None,
            reply_lens.data_ptr() if n else None, lst.data_ptr() if want_list else None,
            cnt.data_ptr() if want_list else None, scratch.data_ptr() if want_list else None,
            _stream_ptr(stream, d)))
    if want_list and own:
        lst = lst[:n]
    return actions, reply_lens, lst, cnt


def _list_args(name: str, plan: str, lst: torch.Tensor, count: torch.Tensor, m: int, n: int,
               device) -> None:
    """A list and its count as ``plan``, the call that produced them, gives them."""
    if not isinstance(lst, torch.Tensor) or not isinstance(count, torch.Tensor) \
            or lst.device != device or count.device != device:
        raise ValueError(f"{name} and its count must be device tensors on {device}")
    if lst.element_size() != 4 or not lst.is_contiguous() or lst.numel() < min(m, n):
        raise ValueError(f"{name} must be a contiguous 4-byte tensor of >= min(m, n) entries")
    if count.element_size() != 8 or count.numel() < 1:
        raise ValueError(f"count must be the 8-byte count of {plan}")


def _build_args(plan: str, base: torch.Tensor, n: int, codes_name: str, codes: torch.Tensor,
                reply_list: torch.Tensor, count: torch.Tensor, engine: torch.Tensor,
                out: torch.Tensor, out_offsets: torch.Tensor, slot_bytes: int, check: bool,
                ip_ids: Optional[torch.Tensor] = None):
    """What rx_reply_build and rx_neigh_build check alike: the code bytes, the
    table, ``out`` / ``out_offsets`` / ``slot_bytes``, the list of ``plan`` and,
    under ``check``, every slot inside ``out`` and ``out`` off ``base``.
    Returns ``(m, out_lens, built)``, the two tensors allocated here."""
    d = base.device
    _same_device(base, out=out, out_offsets=out_offsets)  # (the others: by their own checks)
    _byte_array(codes_name, codes, n, d)
    _engine_tensor(engine, d)
    if not out.is_contiguous() or out.element_size() != 1:
        raise ValueError("out must be a contiguous 1-byte tensor (the replies are written into it)")
    m = out_offsets.numel()
    if out_offsets.element_size() != 8 or out_offsets.is_floating_point() \
            or not out_offsets.is_contiguous() or m > 0xFFFFFFFF:
        raise ValueError("out_offsets must be contiguous 8-byte integers, at most 2^32 - 1")
    if not 0 <= int(slot_bytes) <= 0xFFFF:
        raise ValueError("slot_bytes is at most 65535 (a frame length is a uint16)")
    _list_args("reply_list", plan, reply_list, count, m, n, d)
    if ip_ids is not None:
        _byte_array("ip_ids", ip_ids, m, d, 2)
    if check and m:
        so = out_offsets.view(torch.int64)
        if bool((so < 0).any()) or int(so.max()) + int(slot_bytes) > _nbytes(out):
            raise ValueError("a reply slot [off, off + slot_bytes) runs past out")
        ob, oe = out.data_ptr(), out.data_ptr() + _nbytes(out)
        if ob < base.data_ptr() + _nbytes(base) and base.data_ptr() < oe:
            raise ValueError("out overlaps base: RX frames and reply slots must not overlap")
    return (m, torch.empty(m, dtype=torch.uint16, device=d),
            torch.zeros(1, dtype=torch.int64, device=d))


def rx_reply_build(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                   actions: torch.Tensor, reply_list: torch.Tensor, count: torch.Tensor,
                   engine: torch.Tensor, out: torch.Tensor, out_offsets: torch.Tensor,
                   slot_bytes: int, ip_ids: Optional[torch.Tensor] = None, stream=None,
                   check: bool = True):
    """Write the reply frames rx_reply_plan listed (wc_rx_reply_build): reply
    ``j < min(count, m)``, ``m = out_offsets.numel()``, answers frame
    ``reply_list[j]`` and is written at ``out[out_offsets[j]]``, at most
    ``slot_bytes`` bytes.  ``out`` is a 1-byte device tensor that does not
    overlap ``base``; ``ip_ids`` (optional) holds m uint16 ip->id values as
    stored.  Returns ``(out_lens uint16 -- 0 where no reply was written --,
    built)``, ``built`` a 1-element int64 device tensor.  ``count`` is read on
    the device: no synchronisation.  ``check``: every frame inside ``base`` and
    every slot inside ``out`` (one device reduction and a sync)."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    m, out_lens, built = _build_args("rx_reply_plan", base, n, "actions", actions, reply_list,
                                     count, engine, out, out_offsets, slot_bytes, check, ip_ids)
    with _on_device(d):
        _check("wc_rx_reply_build", _lib.active().wc_rx_reply_build(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(actions),
            reply_list.data_ptr(), count.data_ptr(), engine.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr() if m else None, m, int(slot_bytes),
            ip_ids.data_ptr() if ip_ids is not None and m else None,
            out_lens.data_ptr() if m else None, built.data_ptr(), _stream_ptr(stream, d)))
    return out_lens, built


# --------------------------------------------------------------------------
# RX neighbours (arp_rx / arp_is_at and the NSOL / NADV branches of icmp6_rx /
# icmp6_tx: replies and neighbor_update records).

# enum wc_rx_neigh_action
RN_NONE, RN_MALFORMED = 0, 4
RN_UPDATE4, RN_ARP_IS_AT, RN_NADV, RN_UPDATE6 = range(8, 12)
RN_MASK_REPLY, RN_MASK_UPDATE = 0x600, 0xF00
RN_NAMES = {RN_NONE: "none", RN_MALFORMED: "malformed", RN_UPDATE4: "update4",
            RN_ARP_IS_AT: "arp_is_at", RN_NADV: "nadv", RN_UPDATE6: "update6"}
# struct wc_neigh_update (include/warpcore_gpu/wc_cksum.h): 24 bytes
NEIGH_UPDATE = np.dtype([("af", "u1"), ("action", "u1"), ("mac", "u1", 6), ("addr", "u1", 16)])
assert NEIGH_UPDATE.itemsize == 24


def rx_neigh_plan(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                  actions: torch.Tensor, engine: torch.Tensor, want_replies: bool = True,
                  want_updates: bool = True, stream=None, check: bool = True,
                  scratch: Optional[torch.Tensor] = None):
    """What the reference does with the frames rx_reply_plan marked RR_HOST
    (wc_rx_neigh_plan): ARP and ICMPv6 neighbour solicitations / advertisements.
    ``actions`` are rx_reply_plan's, ``engine`` its RX_ENGINE tensor.  Returns
    ``(nact uint8 RN_*, reply_list, reply_count, update_list, update_count)``:
    the lists / counts as rx_select gives them for ``RN_MASK_REPLY`` and
    ``RN_MASK_UPDATE`` (None, None where not wanted).  Asynchronous; the
    scratch is allocated here unless given."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    _byte_array("actions", actions, n, d)
    _engine_tensor(engine, d)
    nact = torch.empty(n, dtype=torch.uint8, device=d)
    rl = rc = ul = uc = None
    if want_replies:
        rl, _ = _index_list(None, n, d)
        rc = torch.zeros(1, dtype=torch.int64, device=d)
    if want_updates:
        ul, _ = _index_list(None, n, d)
        uc = torch.zeros(1, dtype=torch.int64, device=d)
    scratch = _select_scratch(scratch, n, d) if want_replies or want_updates else None
    with _on_device(d):
        _check("wc_rx_neigh_plan", _lib.active().wc_rx_neigh_plan(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(actions),
            engine.data_ptr(), nact.data_ptr() if n else None,
            rl.data_ptr() if want_replies else None, rc.data_ptr() if want_replies else None,
            ul.data_ptr() if want_updates else None, uc.data_ptr() if want_updates else None,
            scratch.data_ptr() if scratch is not None else None, _stream_ptr(stream, d)))
    return (nact, rl[:n] if want_replies else None, rc, ul[:n] if want_updates else None, uc)


def rx_neigh_updates(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                     nact: torch.Tensor, update_list: torch.Tensor, count: torch.Tensor, m: int,
                     stream=None, check: bool = True) -> torch.Tensor:
    """The neighbor_update records of the frames rx_neigh_plan listed
    (wc_rx_neigh_updates): an ``(m, 24)`` uint8 device tensor, record ``j <
    min(count, m)`` that of frame ``update_list[j]``, the rest all zero (on the
    host: ``.cpu().numpy().view(NEIGH_UPDATE)``).  In ring order: apply them in
    order.  ``count`` is read on the device: no synchronisation."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    m = int(m)
    if not 0 <= m <= 0xFFFFFFFF:
        raise ValueError("m is a uint32")
    d = base.device
    _byte_array("nact", nact, n, d)
    _list_args("update_list", "rx_neigh_plan", update_list, count, m, n, d)
    upd = torch.empty((m, NEIGH_UPDATE.itemsize), dtype=torch.uint8, device=d)
    with _on_device(d):
        _check("wc_rx_neigh_updates", _lib.active().wc_rx_neigh_updates(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(nact),
            update_list.data_ptr(), count.data_ptr(), m, upd.data_ptr() if m else None,
            _stream_ptr(stream, d)))
    return upd


def rx_neigh_build(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                   nact: torch.Tensor, reply_list: torch.Tensor, count: torch.Tensor,
                   engine: torch.Tensor, out: torch.Tensor, out_offsets: torch.Tensor,
                   slot_bytes: int, stream=None, check: bool = True):
    """Write the is-at and advertisement frames rx_neigh_plan listed
    (wc_rx_neigh_build), with rx_reply_build's contract: reply ``j < min(count,
    m)``, ``m = out_offsets.numel()``, answers frame ``reply_list[j]`` at
    ``out[out_offsets[j]]``.  Returns ``(out_lens uint16 -- 0 where no reply was
    written --, built)``."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    m, out_lens, built = _build_args("rx_neigh_plan", base, n, "nact", nact, reply_list, count,
                                     engine, out, out_offsets, slot_bytes, check)
    with _on_device(d):
        _check("wc_rx_neigh_build", _lib.active().wc_rx_neigh_build(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(nact),
            reply_list.data_ptr(), count.data_ptr(), engine.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr() if m else None, m, int(slot_bytes),
            out_lens.data_ptr() if m else None, built.data_ptr(), _stream_ptr(stream, d)))
    return out_lens, built


# --------------------------------------------------------------------------
# RX drain (rx_deliver_ragged -> rx_demux -> rx_reply_plan -> rx_neigh_plan as
# one call: two launches for a ring of at most RX_DRAIN_SMALL frames).

RX_DRAIN_SMALL = 4096  # WC_RX_DRAIN_SMALL


class RxDrain(NamedTuple):
    """The fifteen outputs of rx_drain, in struct wc_rx_drain_out's order."""
    verdicts: torch.Tensor      # uint8 RX_*
    records: torch.Tensor       # (n, 16) uint8: struct wc_rx_record
    drops: torch.Tensor         # 1 int64, accumulated
    sock: torch.Tensor          # uint8 socket ids
    list: torch.Tensor          # uint32, grouped by socket
    start: torch.Tensor         # 256 int64
    actions: torch.Tensor       # uint8 RR_*
    reply_lens: torch.Tensor    # uint16
    reply_list: torch.Tensor    # uint32: RR_MASK_REPLY
    reply_count: torch.Tensor   # 1 int64
    nact: torch.Tensor          # uint8 RN_*
    neigh_reply_list: torch.Tensor   # uint32: RN_MASK_REPLY
    neigh_reply_count: torch.Tensor  # 1 int64
    update_list: torch.Tensor   # uint32: RN_MASK_UPDATE
    update_count: torch.Tensor  # 1 int64


class _DrainOut(ctypes.Structure):  # struct wc_rx_drain_out
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "verdict", "rec", "drops", "sock", "list", "start", "action", "reply_len", "rlist",
        "rcount", "nact", "nrlist", "nrcount", "ulist", "ucount")]


def rx_drain_scratch(n: int) -> int:
    """Bytes of device scratch wc_rx_drain needs for n frames (no GPU)."""
    return int(_lib.active().wc_rx_drain_scratch(int(n)))


def _drain_out(out: Optional[RxDrain], n: int, device) -> RxDrain:
    """rx_drain's fifteen tensors: the caller's, checked, or allocated here."""
    if out is None:
        def lst():
            return _index_list(None, n, device)[0]

        def cnt():
            return torch.zeros(1, dtype=torch.int64, device=device)
        return RxDrain(torch.empty(n, dtype=torch.uint8, device=device),
                       torch.empty((n, RX_RECORD.itemsize), dtype=torch.uint8, device=device),
                       cnt(), torch.empty(n, dtype=torch.uint8, device=device), lst(),
                       torch.zeros(_RX_STARTS, dtype=torch.int64, device=device),
                       torch.empty(n, dtype=torch.uint8, device=device),
                       torch.empty(n, dtype=torch.uint16, device=device), lst(), cnt(),
                       torch.empty(n, dtype=torch.uint8, device=device), lst(), cnt(), lst(), cnt())
    if not isinstance(out, RxDrain):
        raise ValueError("out must be an RxDrain (an earlier call's result)")
    for name in ("verdicts", "sock", "actions", "nact"):
        _byte_array(name, getattr(out, name), n, device)
    _byte_array("reply_lens", out.reply_lens, n, device, 2)
    if not isinstance(out.records, torch.Tensor) or out.records.device != device \
            or not out.records.is_contiguous() or _nbytes(out.records) < n * RX_RECORD.itemsize:
        raise ValueError(f"records must be contiguous (n, 16) bytes on {device}")
    for name in ("list", "reply_list", "neigh_reply_list", "update_list"):
        _index_list(getattr(out, name), n, device)
    for name, most in (("drops", 1), ("start", _RX_STARTS), ("reply_count", 1),
                       ("neigh_reply_count", 1), ("update_count", 1)):
        _byte_array(name, getattr(out, name), most, device, 8)
    return out


def rx_drain(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
             tab: torch.Tensor, ns: int, engine: torch.Tensor, slot_bytes: int = 2048,
             out: Optional[RxDrain] = None, scratch: Optional[torch.Tensor] = None, stream=None,
             check: bool = True) -> RxDrain:
    """The whole per-ring RX plan in one call (wc_rx_drain): every output of
    rx_deliver_ragged, rx_demux (``tab``: rx_socktab_build's bytes for ``ns``
    sockets as a device tensor), rx_reply_plan (with the socket ids) and
    rx_neigh_plan over the same frames, byte for byte -- two launches for at
    most ``RX_DRAIN_SMALL`` frames, the four calls above that.  Returns an
    ``RxDrain``; the lists hold ``max(n, 1)`` entries of which the first
    ``count`` are written, ``drops`` is accumulated (zero in a tuple allocated
    here).  ``out``: an earlier call's ``RxDrain`` to write into again;
    ``scratch``: ``rx_drain_scratch(n)`` bytes, allocated here unless given --
    give both per call in flight when ``stream`` is not the current stream.
    The build calls (rx_reply_build, rx_neigh_updates, rx_neigh_build) take
    its lists and counts unchanged.  Asynchronous."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    _same_device(base, tab=tab)
    if not 0 <= int(ns) <= RX_DEMUX_MAX_SOCKS:
        raise ValueError(f"ns must be 0..{RX_DEMUX_MAX_SOCKS}")
    if not tab.is_contiguous() or _nbytes(tab) < rx_socktab_bytes(ns):
        raise ValueError("tab must hold the rx_socktab_build bytes of ns sockets")
    _engine_tensor(engine, d)
    if not 0 <= int(slot_bytes) <= 0xFFFF:
        raise ValueError("slot_bytes is at most 65535 (a frame length is a uint16)")
    o = _drain_out(out, n, d)
    if scratch is None:
        scratch = _scratch(rx_drain_scratch(n), d)
    elif _nbytes(scratch) < rx_drain_scratch(n) or scratch.device != d:
        raise ValueError(f"scratch must hold rx_drain_scratch(n) bytes on {d}")
    c_out = _DrainOut(*[t.data_ptr() or None for t in o])
    with _on_device(d):
        _check("wc_rx_drain", _lib.active().wc_rx_drain(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, _dev_ptr(tab), int(ns),
            engine.data_ptr(), int(slot_bytes), ctypes.byref(c_out), scratch.data_ptr(),
            _stream_ptr(stream, d)))
    return o


# --------------------------------------------------------------------------
# RX answer (rx_reply_build -> rx_neigh_updates -> rx_neigh_build -> neigh_apply
# as one call: two launches where each list has at most RX_ANSWER_SMALL entries).

RX_ANSWER_SMALL = 4096  # WC_RX_ANSWER_SMALL
RX_ANSWER_SMALL_APPLY = 1024  # WC_RX_ANSWER_SMALL_APPLY: u_m where a table is given


class RxAnswer(NamedTuple):
    """The outputs of rx_answer."""
    reply_lens: torch.Tensor    # uint16, r_m: 0 where no reply was written
    reply_built: torch.Tensor   # 1 int64, written
    neigh_lens: torch.Tensor    # uint16, n_m
    neigh_built: torch.Tensor   # 1 int64, written
    updates: torch.Tensor       # (u_m, 24) uint8: struct wc_neigh_update
    dropped: Optional[torch.Tensor]  # 1 int64, accumulated; None without a table


class _AnswerIo(ctypes.Structure):  # struct wc_rx_answer_io
    _fields_ = [("action", ctypes.c_void_p), ("rlist", ctypes.c_void_p),
                ("rcount", ctypes.c_void_p), ("nact", ctypes.c_void_p),
                ("nrlist", ctypes.c_void_p), ("nrcount", ctypes.c_void_p),
                ("ulist", ctypes.c_void_p), ("ucount", ctypes.c_void_p),
                ("r_out_base", ctypes.c_void_p), ("r_out_off", ctypes.c_void_p),
                ("r_m", ctypes.c_uint32), ("ip_id", ctypes.c_void_p),
                ("r_out_len", ctypes.c_void_p), ("r_built", ctypes.c_void_p),
                ("n_out_base", ctypes.c_void_p), ("n_out_off", ctypes.c_void_p),
                ("n_m", ctypes.c_uint32), ("n_out_len", ctypes.c_void_p),
                ("n_built", ctypes.c_void_p), ("u_m", ctypes.c_uint32),
                ("upd", ctypes.c_void_p), ("tab", ctypes.c_void_p),
                ("dropped", ctypes.c_void_p)]


def rx_answer_scratch(u_m: int) -> int:
    """Bytes of device scratch wc_rx_answer needs for u_m update records when a
    table is given (no GPU)."""
    return int(_lib.active().wc_rx_answer_scratch(int(u_m)))


def rx_answer(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
              plan, engine: torch.Tensor, reply_out: torch.Tensor, reply_offsets: torch.Tensor,
              neigh_out: torch.Tensor, neigh_offsets: torch.Tensor, u_m: int,
              slot_bytes: int = 2048, ip_ids: Optional[torch.Tensor] = None,
              tab: Optional[torch.Tensor] = None, out: Optional[RxAnswer] = None,
              scratch: Optional[torch.Tensor] = None, stream=None,
              check: bool = True) -> RxAnswer:
    """Everything behind a drain in one call (wc_rx_answer): the outputs of
    rx_reply_build (``reply_out`` / ``reply_offsets`` / ``ip_ids``),
    rx_neigh_updates (``u_m`` records), rx_neigh_build (``neigh_out`` /
    ``neigh_offsets``) and, where ``tab`` is given, neigh_apply on it, byte for
    byte -- two launches where the two offset arrays and ``u_m`` are at most
    ``RX_ANSWER_SMALL`` (``u_m`` at most ``RX_ANSWER_SMALL_APPLY`` with a table),
    the four calls above that.  ``plan``: an ``RxDrain``, or
    the eight tensors ``(actions, reply_list, reply_count, nact,
    neigh_reply_list, neigh_reply_count, update_list, update_count)``.  The reply
    slots and the neighbour slots must not overlap each other.  Returns an
    ``RxAnswer``; both built counts are written, ``dropped`` is accumulated
    (zero in a tuple allocated here).  ``out``: an earlier call's ``RxAnswer`` to
    write into again; ``scratch``: ``rx_answer_scratch(u_m)`` bytes, allocated
    here unless given -- give both per call in flight when ``stream`` is not the
    current stream.  Asynchronous; calls on one table are ordered by the
    caller."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    if isinstance(plan, RxDrain):
        plan = (plan.actions, plan.reply_list, plan.reply_count, plan.nact,
                plan.neigh_reply_list, plan.neigh_reply_count, plan.update_list,
                plan.update_count)
    if not isinstance(plan, (tuple, list)) or len(plan) != 8:
        raise ValueError("plan must be an RxDrain or its eight tensors (actions, reply_list, "
                         "reply_count, nact, neigh_reply_list, neigh_reply_count, update_list, "
                         "update_count)")
    actions, rlist, rcount, nact, nrlist, nrcount, ulist, ucount = plan
    r_m, r_lens, r_built = _build_args("rx_reply_plan", base, n, "actions", actions, rlist, rcount,
                                       engine, reply_out, reply_offsets, slot_bytes, check, ip_ids)
    n_m, n_lens, n_built = _build_args("rx_neigh_plan", base, n, "nact", nact, nrlist, nrcount,
                                       engine, neigh_out, neigh_offsets, slot_bytes, check)
    u_m = int(u_m)
    if not 0 <= u_m <= (0xFFFFFFFF if tab is None else _NEIGH_APPLY_MAX):
        raise ValueError("u_m is a uint32, and at most 2^31 with a table")
    _list_args("update_list", "rx_neigh_plan", ulist, ucount, u_m, n, d)
    if tab is not None:
        _neigh_tab(tab)
        if tab.device != d:
            raise ValueError(f"tab is on {tab.device}, base on {d}")
    if out is None:
        out = RxAnswer(r_lens, r_built, n_lens, n_built,
                       torch.empty((u_m, NEIGH_UPDATE.itemsize), dtype=torch.uint8, device=d),
                       _bad_counter(None, d) if tab is not None else None)
    else:
        if not isinstance(out, RxAnswer):
            raise ValueError("out must be an RxAnswer (an earlier call's result)")
        _byte_array("reply_lens", out.reply_lens, r_m, d, 2)
        _byte_array("neigh_lens", out.neigh_lens, n_m, d, 2)
        _byte_array("reply_built", out.reply_built, 1, d, 8)
        _byte_array("neigh_built", out.neigh_built, 1, d, 8)
        if not isinstance(out.updates, torch.Tensor) or out.updates.device != d \
                or not out.updates.is_contiguous() \
                or _nbytes(out.updates) < u_m * NEIGH_UPDATE.itemsize:
            raise ValueError(f"updates must be contiguous (u_m, 24) bytes on {d}")
        if tab is not None:
            out = out._replace(dropped=_bad_counter(out.dropped, d, "dropped"))
    need = rx_answer_scratch(u_m) if tab is not None else 0
    if scratch is None:
        scratch = _scratch(need, d)
    elif _nbytes(scratch) < need or scratch.device != d:
        raise ValueError(f"scratch must hold rx_answer_scratch(u_m) bytes on {d}")

    def ptr(t, some=True):
        return t.data_ptr() if t is not None and some else None
    io = _AnswerIo(ptr(actions), ptr(rlist), ptr(rcount), ptr(nact), ptr(nrlist), ptr(nrcount),
                   ptr(ulist), ptr(ucount),
                   ptr(reply_out), ptr(reply_offsets, r_m), r_m, ptr(ip_ids, r_m),
                   ptr(out.reply_lens, r_m), ptr(out.reply_built),
                   ptr(neigh_out), ptr(neigh_offsets, n_m), n_m, ptr(out.neigh_lens, n_m),
                   ptr(out.neigh_built), u_m, ptr(out.updates, u_m), ptr(tab),
                   ptr(out.dropped, tab is not None))
    with _on_device(d):
        _check("wc_rx_answer", _lib.active().wc_rx_answer(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, engine.data_ptr(),
            int(slot_bytes), ctypes.byref(io), scratch.data_ptr(), _stream_ptr(stream, d)))
    return out


# --------------------------------------------------------------------------
# RX echo (the delivered datagrams of the switched-on sockets as a TX batch for
# tx_pump: descriptors, destinations and payloads in one launch).

RX_ECHO_MAX = 65536  # WC_RX_ECHO_MAX
ECHO_OFF = 0xFFFF    # WC_ECHO_OFF
EC_ECHO, EC_NONE, EC_SHORT, EC_NO_ROOM, EC_STALE = 0, 4, 8, 9, 10
EC_NAMES = {EC_ECHO: "echo", EC_NONE: "none", EC_SHORT: "short", EC_NO_ROOM: "no_room",
            EC_STALE: "stale"}
EC_MASK_SKIPPED = (1 << EC_SHORT) | (1 << EC_NO_ROOM) | (1 << EC_STALE)


class RxEcho(NamedTuple):
    """The outputs of rx_echo, in struct wc_rx_echo_out's order."""
    descs: torch.Tensor      # (m, 8) uint8: struct wc_tx_desc
    dsts: torch.Tensor       # (m, 24) uint8: struct wc_tx_dst
    af: torch.Tensor         # uint8: 4 / 6, 0 for an inert entry
    status: torch.Tensor     # uint8 EC_*
    src: Optional[torch.Tensor]     # uint32: the ring index of entry j, 0xFFFFFFFF without one
    tx_off: Optional[torch.Tensor]  # int64, in-place mode only: the pump's offsets
    count: torch.Tensor      # 1 int64, written: E
    skipped: Optional[torch.Tensor]  # 1 int64, accumulated


class _EchoOut(ctypes.Structure):  # struct wc_rx_echo_out
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "desc", "dsts", "af", "status", "src", "tx_off", "count", "skipped")]


def _echo_out(out: Optional[RxEcho], m: int, in_place: bool, device) -> RxEcho:
    """rx_echo's tensors: the caller's, checked, or allocated here."""
    if out is None:
        def arr(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=device)
        return RxEcho(arr((m, 8), torch.uint8), arr((m, 24), torch.uint8), arr(m, torch.uint8),
                      arr(m, torch.uint8), arr(m, torch.uint32),
                      arr(m, torch.int64) if in_place else None,
                      torch.zeros(1, dtype=torch.int64, device=device),
                      torch.zeros(1, dtype=torch.int64, device=device))
    if not isinstance(out, RxEcho):
        raise ValueError("out must be an RxEcho (an earlier call's result)")
    for name, size in (("descs", 8), ("dsts", 24)):
        t = getattr(out, name)
        if not isinstance(t, torch.Tensor) or t.device != device or not t.is_contiguous() \
                or t.element_size() != 1 or _nbytes(t) < m * size:
            raise ValueError(f"{name} must be contiguous (m, {size}) bytes on {device}")
    _byte_array("af", out.af, m, device)
    _byte_array("status", out.status, m, device)
    if out.src is not None:
        _byte_array("src", out.src, m, device, 4)
    if in_place != (out.tx_off is not None):
        raise ValueError("tx_off goes with in-place mode alone")
    if in_place:
        _byte_array("tx_off", out.tx_off, m, device, 8)
    _byte_array("count", out.count, 1, device, 8)
    if out.skipped is not None:
        _byte_array("skipped", out.skipped, 1, device, 8)
    return out


def rx_echo(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor, plan,
            echo_map: torch.Tensor, m: Optional[int] = None,
            out_base: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
            out_slot_bytes: int = 2048, ip_ids: Optional[torch.Tensor] = None,
            out: Optional[RxEcho] = None, stream=None, check: bool = True) -> RxEcho:
    """The delivered datagrams of the switched-on sockets as a TX batch
    (wc_rx_echo, one launch): inetd's port 7 on the device.  ``plan``: an
    ``RxDrain``, or the three tensors ``(records, list, start)`` of rx_demux;
    ``echo_map``: one 2-byte entry per RX socket, the ``TX_SOCK`` index it
    answers from, or ``ECHO_OFF``.  Entry j of the result is the j-th frame of
    the switched-on sockets' runs, sockets ascending: a descriptor with ``dst =
    j``, a destination (the frame's IP source and UDP source port; ``dmac`` a
    placeholder that tx_pump's resolve overwrites), ``af`` and an ``EC_*``
    status.  Copy mode -- ``out_base`` / ``out_offsets`` given, ``m`` their
    count: the payloads are copied behind the header space of each slot.
    In-place mode -- neither given, ``m`` required: ``tx_off`` holds the offsets
    to hand tx_pump with ``base`` itself, so that it writes its headers in front
    of the received payloads (pass it a slot length reduced by 40).  All ``m``
    entries are written (``src`` and ``skipped`` may be None in a tuple handed
    in), the ones past ``count`` and the skipped ones so that
    tx_pump refuses them (``TX_MALFORMED``, counted in its ``errors``): call it
    with all ``m``.  ``count`` is written, ``skipped`` accumulated (zero in a
    tuple allocated here).  ``ip_ids``: ``m`` uint16, the IPv4 ids as stored.
    Asynchronous with ``check=False``; under ``check`` (the default) the frame
    and slot offsets are reduced on the device and read back first, which
    synchronises -- pass ``check=False`` where drain -> echo -> pump must run
    with no host read in between.  No scratch."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, indexed=True)
    d = base.device
    if isinstance(plan, RxDrain):
        plan = (plan.records, plan.list, plan.start)
    if not isinstance(plan, (tuple, list)) or len(plan) != 3:
        raise ValueError("plan must be an RxDrain or the three tensors (records, list, start)")
    records, lst, start = plan
    if not isinstance(records, torch.Tensor) or records.device != d or not records.is_contiguous() \
            or _nbytes(records) < n * RX_RECORD.itemsize:
        raise ValueError(f"records must be contiguous (n, 16) bytes on {d}")
    _index_list(lst, n, d)
    _byte_array("start", start, _RX_STARTS, d, 8)
    if not isinstance(echo_map, torch.Tensor) or echo_map.device != d \
            or echo_map.element_size() != 2 or echo_map.is_floating_point() \
            or not echo_map.is_contiguous() or echo_map.numel() > RX_DEMUX_MAX_SOCKS:
        raise ValueError(f"echo_map must be at most {RX_DEMUX_MAX_SOCKS} contiguous 2-byte "
                         f"integers on {d}")
    ns = echo_map.numel()
    in_place = out_base is None
    if (out_base is None) != (out_offsets is None):
        raise ValueError("out_base and out_offsets go together (neither: in-place mode)")
    if in_place:
        if m is None:
            raise ValueError("in-place mode needs m, the number of entries")
        m = int(m)
    else:
        if not out_base.is_contiguous() or out_base.element_size() != 1 or out_base.device != d:
            raise ValueError(f"out_base must be a contiguous 1-byte tensor on {d}")
        if out_offsets.element_size() != 8 or out_offsets.is_floating_point() \
                or not out_offsets.is_contiguous() or out_offsets.device != d:
            raise ValueError(f"out_offsets must be contiguous 8-byte integers on {d}")
        if m is not None and int(m) != out_offsets.numel():
            raise ValueError("m is the number of out_offsets")
        m = out_offsets.numel()
    if not 0 <= m <= RX_ECHO_MAX:
        raise ValueError(f"m is at most {RX_ECHO_MAX} (a descriptor's dst is 16 bits)")
    if not 0 <= int(out_slot_bytes) <= 0xFFFF:
        raise ValueError("out_slot_bytes is at most 65535")
    if ip_ids is not None:
        _byte_array("ip_ids", ip_ids, m, d, 2)
    if check and m and not in_place:
        oo = out_offsets.view(torch.int64)
        if bool((oo < 0).any()) or int(oo.max()) + int(out_slot_bytes) > _nbytes(out_base):
            raise ValueError("a slot [off, off + out_slot_bytes) runs past out_base")
        ob, oe = out_base.data_ptr(), out_base.data_ptr() + _nbytes(out_base)
        if ob < base.data_ptr() + _nbytes(base) and base.data_ptr() < oe:
            raise ValueError("out_base overlaps base: the slots must not overlap the RX buffer")
    o = _echo_out(out, m, in_place, d)

    def ptr(t, some=True):
        return (t.data_ptr() or None) if t is not None and some else None
    c_out = _EchoOut(ptr(o.descs), ptr(o.dsts), ptr(o.af), ptr(o.status), ptr(o.src),
                     ptr(o.tx_off, m), ptr(o.count), ptr(o.skipped))
    rx = n != 0 and ns != 0
    with _on_device(d):
        _check("wc_rx_echo", _lib.active().wc_rx_echo(
            ptr(base, rx), ptr(offsets, rx), ptr(frame_lens, rx), n, ptr(records, rx),
            ptr(lst, rx), ptr(start, rx), ptr(echo_map, rx), ns, ptr(ip_ids, m),
            ptr(out_base, m), ptr(out_offsets, m), int(out_slot_bytes), m, ctypes.byref(c_out),
            _stream_ptr(stream, d)))
    return o


# --------------------------------------------------------------------------
# TX seal (what mk_ip4_hdr and udp_tx store, computed and stored on the device).

# enum wc_tx_status (include/warpcore_gpu/wc_cksum.h)
TX_SEALED, TX_SEALED_ZERO_UDP, TX_IP_ONLY, TX_NOT_UDP, TX_NOT_IP, TX_BAD_VERSION, \
    TX_MALFORMED, TX_TRUNCATED = range(8)
TX_NAMES = ("sealed", "sealed_zero_udp", "ip_only", "not_udp", "not_ip", "bad_version",
            "malformed", "truncated")
TX_ERRORS = (TX_BAD_VERSION, TX_MALFORMED, TX_TRUNCATED)
_TX_ZERO_UDP_CKSUM, _TX_NO_STORE = 1, 2


def tx_seal_ragged(base: torch.Tensor, offsets: torch.Tensor, frame_lens: torch.Tensor,
                   zero_udp: bool = False, store: bool = True, stream=None,
                   check: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                torch.Tensor]:
    """Seal every Ethernet frame ``base[off[i] : off[i] + frame_len[i]]`` in
    place (wc_tx_seal_ragged): the IPv4 header checksum and the UDP checksum,
    each computed with its field taken as 0 and stored raw into the frame
    (``zero_udp``: udp->cksum = 0, the zero-checksum socket; ``store=False``:
    compute only, ``base`` untouched).  The frames must not overlap.  Returns
    (uint8 status ``TX_*`` per frame, uint16 header checksums, uint16 UDP
    checksums -- 0 where none is computed --, int64 count of ``TX_ERRORS``
    frames)."""
    n = _check_ragged(base, offsets, frame_lens, KIND_IP, check, in_place=True)
    status = torch.empty(n, dtype=torch.uint8, device=base.device)
    hdr = torch.empty(n, dtype=torch.uint16, device=base.device)
    udp = torch.empty(n, dtype=torch.uint16, device=base.device)
    errors = torch.zeros(1, dtype=torch.int64, device=base.device)
    flags = (_TX_ZERO_UDP_CKSUM if zero_udp else 0) | (0 if store else _TX_NO_STORE)
    with _on_device(base.device):
        _check("wc_tx_seal_ragged", _lib.active().wc_tx_seal_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(frame_lens), n, flags,
            status.data_ptr(), hdr.data_ptr(), udp.data_ptr(), errors.data_ptr(),
            _stream_ptr(stream, base.device)))
    return status, hdr, udp, errors


def _in_place_bytes(func: str, buf: np.ndarray) -> np.ndarray:
    """``buf``'s own bytes, flat, for a host call that writes the frames."""
    if not isinstance(buf, np.ndarray) or not buf.flags["C_CONTIGUOUS"] \
            or not buf.flags["WRITEABLE"] or buf.dtype.itemsize != 1:
        raise ValueError(f"{func} writes the frames in place: buf must be a writable "
                         "C-contiguous 1-byte numpy array")
    return buf.reshape(-1).view(np.uint8)


def tx_seal_host(buf: np.ndarray, offsets: np.ndarray, frame_lens: np.ndarray,
                 zero_udp: bool = False) -> Tuple[np.ndarray, int]:
    """tx_seal_ragged over host memory (wc_tx_seal_host, synchronous): the
    frames in ``buf`` are sealed in place; (uint8 status codes, error count)."""
    flat = _in_place_bytes("tx_seal_host", buf)
    _, off, lens = _host_batch_args(flat, offsets, frame_lens)
    status = np.empty(off.size, dtype=np.uint8)
    errors = ctypes.c_uint64()
    _check("wc_tx_seal_host", _lib.active().wc_tx_seal_host(
        flat.ctypes.data, flat.size, off.ctypes.data, lens.ctypes.data, off.size,
        _TX_ZERO_UDP_CKSUM if zero_udp else 0, status.ctypes.data, ctypes.byref(errors)))
    return status, int(errors.value)


# --------------------------------------------------------------------------
# TX build (the per-iov body of udp_tx: Ethernet / IP / UDP headers written
# from a socket table, checksums included).

# struct wc_tx_sock / wc_tx_dst / wc_tx_desc (include/warpcore_gpu/wc_cksum.h)
TX_SOCK = np.dtype([("af", "u1"), ("flags", "u1"), ("lport", "<u2"), ("rport", "<u2"),
                    ("smac", "u1", 6), ("dmac", "u1", 6), ("pad", "u1", 2),
                    ("laddr", "u1", 16), ("raddr", "u1", 16)])
TX_DST = np.dtype([("addr", "u1", 16), ("dmac", "u1", 6), ("port", "<u2")])
TX_DESC = np.dtype([("data_len", "<u2"), ("ip_id", "<u2"), ("sock", "u1"), ("tos", "u1"),
                    ("dst", "<u2")])
assert (TX_SOCK.itemsize, TX_DST.itemsize, TX_DESC.itemsize) == (52, 24, 8)
TX_SOCK_CONNECTED, TX_SOCK_ECN = 1, 2
TX_BUILD_MAX_SOCKS = 256
_TX_BUILD_MAX_DSTS = 65536


def tx_socks_check(socks: np.ndarray) -> None:
    """``ValueError`` for a socket array wc_tx_socks_check refuses: more than
    256 entries, an af other than 4 / 6, unknown flag bits.  No GPU."""
    socks = np.ascontiguousarray(socks, dtype=TX_SOCK).reshape(-1)
    rc = _lib.active().wc_tx_socks_check(socks.ctypes.data if socks.size else None, socks.size)
    if rc == _WC_EINVAL:
        raise ValueError(f"TX socket array: at most {TX_BUILD_MAX_SOCKS} entries, af 4 or 6, "
                         "flags of TX_SOCK_CONNECTED | TX_SOCK_ECN")
    _check("wc_tx_socks_check", rc)


def _table_tensor(name: str, t: torch.Tensor, dtype: np.dtype, most: int, device) -> int:
    """Entries of a device table given as its contiguous bytes."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise ValueError(f"{name} must be a device tensor on {device}")
    if not t.is_contiguous() or _nbytes(t) % dtype.itemsize:
        raise ValueError(f"{name} must be the contiguous bytes of {dtype.itemsize}-byte entries")
    k = _nbytes(t) // dtype.itemsize
    if k > most:
        raise ValueError(f"{name}: at most {most} entries")
    return k


def tx_build_ragged(base: torch.Tensor, offsets: torch.Tensor, descs: torch.Tensor,
                    socks: torch.Tensor, dsts: Optional[torch.Tensor], slot_bytes: int,
                    zero_udp: bool = False, store: bool = True, stream=None,
                    errors: Optional[torch.Tensor] = None):
    """Write the Ethernet, IP and UDP headers of every frame in place
    (wc_tx_build_ragged): frame ``i`` starts at ``base[off[i]]``, may use
    ``slot_bytes`` bytes and already holds its payload behind the 42 (IPv4) or
    62 (IPv6) header bytes.  ``descs`` / ``socks`` / ``dsts``: device tensors
    holding the bytes of ``TX_DESC`` / ``TX_SOCK`` / ``TX_DST`` arrays
    (``torch.from_numpy(a.view(np.uint8))``; ``dsts`` may be None).  Returns
    (uint16 frame lengths -- 0 for an error frame --, uint8 status ``TX_*``,
    uint16 IPv4 header checksums, uint16 UDP checksums, int64 count of
    ``TX_ERRORS`` frames; a given ``errors`` tensor is accumulated into).  The
    caller keeps every frame's slot inside ``base``."""
    _same_device(base, offsets=offsets, descs=descs, socks=socks, dsts=dsts)
    d = base.device
    if not base.is_contiguous() or base.element_size() != 1:
        raise ValueError("base must be a contiguous 1-byte tensor (the frames are written in place)")
    n = offsets.numel()
    if offsets.element_size() != 8 or offsets.is_floating_point() or not offsets.is_contiguous():
        raise ValueError("offsets must be contiguous 8-byte integers")
    if not descs.is_contiguous() or _nbytes(descs) != n * TX_DESC.itemsize:
        raise ValueError("descs must be the contiguous bytes of one TX_DESC per frame")
    ns = _table_tensor("socks", socks, TX_SOCK, TX_BUILD_MAX_SOCKS, d)
    ndst = 0 if dsts is None else _table_tensor("dsts", dsts, TX_DST, _TX_BUILD_MAX_DSTS, d)
    if not 0 <= int(slot_bytes) <= 0xFFFFFFFF:
        raise ValueError("slot_bytes is a uint32")
    frame_len = torch.empty(n, dtype=torch.uint16, device=d)
    status = torch.empty(n, dtype=torch.uint8, device=d)
    hdr = torch.empty(n, dtype=torch.uint16, device=d)
    udp = torch.empty(n, dtype=torch.uint16, device=d)
    errors = _bad_counter(errors, d, "errors")
    flags = (_TX_ZERO_UDP_CKSUM if zero_udp else 0) | (0 if store else _TX_NO_STORE)
    with _on_device(d):
        _check("wc_tx_build_ragged", _lib.active().wc_tx_build_ragged(
            _dev_ptr(base), _dev_ptr(offsets), _dev_ptr(descs), n,
            socks.data_ptr() if ns else None, ns, dsts.data_ptr() if ndst else None, ndst,
            int(slot_bytes), flags, frame_len.data_ptr(), status.data_ptr(), hdr.data_ptr(),
            udp.data_ptr(), errors.data_ptr(), _stream_ptr(stream, d)))
    return frame_len, status, hdr, udp, errors


# --------------------------------------------------------------------------
# TX neighbours (neighbor.c's cache on the device, who_has for a whole
# destination table, arp_who_has / icmp6_nsol frames).

NEIGH_TAB_MIN_CAP, NEIGH_TAB_MAX_CAP = 64, 1 << 20
# enum wc_neigh_resolve, enum wc_tx_hold
NR_READY, NR_BAD_AF, NR_MISS, NR_MISS_DUP = 0, 4, 8, 9
NR_MASK_SOLICIT, NR_MASK_MISS = 0x100, 0x300
NR_NAMES = {NR_READY: "ready", NR_BAD_AF: "bad_af", NR_MISS: "miss", NR_MISS_DUP: "miss_dup"}
TH_READY, TH_MALFORMED, TH_HELD = 0, 4, 8
TH_MASK_HELD = 0x100
TH_NAMES = {TH_READY: "ready", TH_MALFORMED: "malformed", TH_HELD: "held"}
_NEIGH_APPLY_MAX = 1 << 31


def neigh_tab_bytes(cap: int) -> int:
    """Bytes of a neighbour table of ``cap`` entries (wc_neigh_tab_bytes, no
    GPU).  ``ValueError`` unless cap is a power of two in [64, 2^20]."""
    cap = int(cap)
    nb = int(_lib.active().wc_neigh_tab_bytes(cap)) if 0 <= cap <= 0xFFFFFFFF else 0
    if nb == 0:
        raise ValueError(f"cap must be a power of two in [{NEIGH_TAB_MIN_CAP}, {NEIGH_TAB_MAX_CAP}]")
    return nb


def _neigh_tab(tab: torch.Tensor) -> None:
    if not isinstance(tab, torch.Tensor) or not tab.is_cuda or not tab.is_contiguous() \
            or tab.data_ptr() % 16 or _nbytes(tab) < 64 + 32 * NEIGH_TAB_MIN_CAP:
        raise ValueError("tab must be the contiguous, 16-byte aligned device tensor neigh_tab_init gave")


def neigh_tab_init(cap: int, device=None, stream=None,
                   tab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """An empty neighbour table of ``cap`` entries on ``device``
    (wc_neigh_tab_init): a uint8 device tensor of ``neigh_tab_bytes(cap)``
    bytes, allocated here unless ``tab`` -- an earlier one of at least that size
    -- is given; initialising a table again is the flush.  Asynchronous."""
    nb = neigh_tab_bytes(cap)
    if tab is None:
        if device is None:
            raise ValueError("neigh_tab_init needs a device or a tab")
        tab = torch.empty(nb, dtype=torch.uint8, device=device)
    _neigh_tab(tab)
    if _nbytes(tab) < nb:
        raise ValueError(f"tab holds fewer than neigh_tab_bytes({cap}) = {nb} bytes")
    with _on_device(tab.device):
        _check("wc_neigh_tab_init", _lib.active().wc_neigh_tab_init(
            tab.data_ptr(), int(cap), _stream_ptr(stream, tab.device)))
    return tab


def neigh_apply(tab: torch.Tensor, updates: torch.Tensor, count: torch.Tensor,
                m: Optional[int] = None, dropped: Optional[torch.Tensor] = None,
                stream=None) -> torch.Tensor:
    """neighbor_update for the records ``j < min(count, m)`` of ``updates`` (the
    ``(m, 24)`` uint8 tensor rx_neigh_updates gives; ``m`` defaults to its
    rows), applied to ``tab`` as if in order (wc_neigh_apply).  ``count`` is
    read on the device.  Returns ``dropped``, a 1-element int64 device tensor
    (accumulated into when given): the records with an af other than 0 / 4 / 6
    or with a key a full table could not take.  Asynchronous; the scratch is
    allocated here.  Calls on one table are ordered by the caller."""
    _neigh_tab(tab)
    d = tab.device
    if not isinstance(updates, torch.Tensor) or updates.device != d or not updates.is_contiguous() \
            or _nbytes(updates) % NEIGH_UPDATE.itemsize:
        raise ValueError(f"updates must be the contiguous bytes of NEIGH_UPDATE records on {d}")
    rows = _nbytes(updates) // NEIGH_UPDATE.itemsize
    m = rows if m is None else int(m)
    if not 0 <= m <= min(rows, _NEIGH_APPLY_MAX):
        raise ValueError("m is at most the records in updates, and at most 2^31")
    if not isinstance(count, torch.Tensor) or count.device != d or count.element_size() != 8 \
            or count.numel() < 1:
        raise ValueError(f"count must be an 8-byte count on {d}")
    dropped = _bad_counter(dropped, d, "dropped")
    scratch = _scratch(4 * m, d)
    with _on_device(d):
        _check("wc_neigh_apply", _lib.active().wc_neigh_apply(
            tab.data_ptr(), updates.data_ptr() if m else None, count.data_ptr(), m,
            dropped.data_ptr(), scratch.data_ptr(), _stream_ptr(stream, d)))
    return dropped


def _host_tab(tab: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(tab).reshape(-1).view(np.uint8)
    if t.size < 64 + 32 * NEIGH_TAB_MIN_CAP or t.size % 4:
        raise ValueError("tab must be a host copy of a neighbour table (tab.cpu().numpy())")
    return np.ascontiguousarray(t.view(np.uint32))  # 4-byte aligned


def neigh_tab_lookup(tab: np.ndarray, af: int, addr) -> Optional[bytes]:
    """The MAC ``tab`` -- a host copy of a neighbour table -- holds for ``(af,
    addr)``, or None (wc_neigh_tab_lookup: the device's own hash and probe, on
    the host).  ``ValueError`` for an af other than 4 / 6 or bytes that are no
    table."""
    t = _host_tab(tab)
    if af not in (4, 6):
        raise ValueError("af is 4 or 6")
    a = _addr_bytes(af, addr)
    mac = (ctypes.c_uint8 * 6)()
    rc = _lib.active().wc_neigh_tab_lookup(t.ctypes.data, int(af), a.ctypes.data, mac)
    if rc == _WC_EINVAL:
        raise ValueError("not a neighbour table: neigh_tab_init did not write these bytes")
    _check("wc_neigh_tab_lookup", min(rc, 0))
    return bytes(mac) if rc == 1 else None


def neigh_tab_stats(tab: np.ndarray) -> Tuple[int, int]:
    """``(cap, used)`` of a host copy of a neighbour table (wc_neigh_tab_stats)."""
    t = _host_tab(tab)
    cap, used = ctypes.c_uint32(), ctypes.c_uint32()
    rc = _lib.active().wc_neigh_tab_stats(t.ctypes.data, ctypes.byref(cap), ctypes.byref(used))
    if rc == _WC_EINVAL:
        raise ValueError("not a neighbour table: neigh_tab_init did not write these bytes")
    _check("wc_neigh_tab_stats", rc)
    return int(cap.value), int(used.value)


def tx_resolve_scratch(ndst: int) -> int:
    """Bytes of device scratch wc_tx_resolve needs for ndst destinations (no GPU)."""
    return int(_lib.active().wc_tx_resolve_scratch(int(ndst)))


def tx_resolve(tab: torch.Tensor, dsts: torch.Tensor, af: torch.Tensor, want_list: bool = True,
               stream=None):
    """The batched who_has (wc_tx_resolve): for every entry of ``dsts`` (the
    bytes of a ``TX_DST`` array on the device, at most 65536) whose address, read
    as family ``af[k]`` (uint8, 4 or 6), ``tab`` resolves to a MAC that is not
    broadcast, that MAC is written into its ``dmac``; for the others ``dmac`` is
    written ff x 6.  Returns ``(state uint8 NR_*, list, count)``: the ascending
    indices with ``NR_MISS`` -- one per distinct unresolved address, the ones to
    solicit -- as rx_select gives them (None, None with ``want_list=False``).
    Asynchronous; the scratch is allocated here."""
    _neigh_tab(tab)
    d = tab.device
    ndst = _table_tensor("dsts", dsts, TX_DST, _TX_BUILD_MAX_DSTS, d)
    _byte_array("af", af, ndst, d)
    state = torch.empty(ndst, dtype=torch.uint8, device=d)
    lst = cnt = None
    if want_list:
        lst, _ = _index_list(None, ndst, d)
        cnt = torch.zeros(1, dtype=torch.int64, device=d)
    scratch = _scratch(tx_resolve_scratch(ndst), d)
    with _on_device(d):
        _check("wc_tx_resolve", _lib.active().wc_tx_resolve(
            tab.data_ptr(), dsts.data_ptr() if ndst else None, af.data_ptr() if ndst else None,
            ndst, state.data_ptr() if ndst else None, lst.data_ptr() if want_list else None,
            cnt.data_ptr() if want_list else None, scratch.data_ptr(), _stream_ptr(stream, d)))
    return state, (lst[:ndst] if want_list else None), cnt


def tx_hold_plan(descs: torch.Tensor, socks: torch.Tensor, state: Optional[torch.Tensor],
                 af: Optional[torch.Tensor], want_list: bool = True, stream=None,
                 scratch: Optional[torch.Tensor] = None):
    """Which frames of a TX batch wait for a neighbour (wc_tx_hold_plan):
    ``descs`` / ``socks`` as tx_build_ragged takes them, ``state`` / ``af`` the
    per-destination bytes of tx_resolve (None, None without destinations).
    Returns ``(hold uint8 TH_*, list, count)``: the ``TH_HELD`` frames as
    rx_select gives them (None, None with ``want_list=False``).  Asynchronous."""
    if not isinstance(descs, torch.Tensor) or not descs.is_cuda:
        raise ValueError("descs must be a device tensor")
    d = descs.device
    if not descs.is_contiguous() or _nbytes(descs) % TX_DESC.itemsize:
        raise ValueError("descs must be the contiguous bytes of TX_DESC entries")
    n = _nbytes(descs) // TX_DESC.itemsize
    ns = _table_tensor("socks", socks, TX_SOCK, TX_BUILD_MAX_SOCKS, d)
    if (state is None) != (af is None):
        raise ValueError("state and af go together")
    ndst = 0
    if state is not None:
        ndst = state.numel()
        if ndst > _TX_BUILD_MAX_DSTS:
            raise ValueError(f"at most {_TX_BUILD_MAX_DSTS} destinations")
        _byte_array("state", state, ndst, d)
        _byte_array("af", af, ndst, d)
    hold = torch.empty(n, dtype=torch.uint8, device=d)
    lst = cnt = None
    if want_list:
        lst, _ = _index_list(None, n, d)
        cnt = torch.zeros(1, dtype=torch.int64, device=d)
        scratch = _select_scratch(scratch, n, d)
    with _on_device(d):
        _check("wc_tx_hold_plan", _lib.active().wc_tx_hold_plan(
            descs.data_ptr() if n else None, n, socks.data_ptr() if ns else None, ns,
            state.data_ptr() if ndst else None, af.data_ptr() if ndst else None, ndst,
            hold.data_ptr() if n else None, lst.data_ptr() if want_list else None,
            cnt.data_ptr() if want_list else None, scratch.data_ptr() if want_list else None,
            _stream_ptr(stream, d)))
    return hold, (lst[:n] if want_list else None), cnt


def tx_solicit_build(dsts: torch.Tensor, af: torch.Tensor, miss_list: torch.Tensor,
                     count: torch.Tensor, engine: torch.Tensor, out: torch.Tensor,
                     out_offsets: torch.Tensor, slot_bytes: int, stream=None, check: bool = True):
    """Write the ARP who-has and neighbour solicitation frames for the
    destinations tx_resolve listed (wc_tx_solicit_build), with rx_neigh_build's
    contract: frame ``j < min(count, m)``, ``m = out_offsets.numel()``, solicits
    ``dsts[miss_list[j]]`` at ``out[out_offsets[j]]``.  Returns ``(out_lens uint16
    -- 0 where no frame was written --, built)``."""
    d = out.device if isinstance(out, torch.Tensor) else None
    ndst = _table_tensor("dsts", dsts, TX_DST, _TX_BUILD_MAX_DSTS, d)
    _byte_array("af", af, ndst, d)
    m, out_lens, built = _build_args("tx_resolve", dsts, ndst, "af", af, miss_list, count, engine,
                                     out, out_offsets, slot_bytes, check)
    with _on_device(d):
        _check("wc_tx_solicit_build", _lib.active().wc_tx_solicit_build(
            dsts.data_ptr() if ndst else None, af.data_ptr() if ndst else None, ndst,
            miss_list.data_ptr(), count.data_ptr(), engine.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr() if m else None, m, int(slot_bytes),
            out_lens.data_ptr() if m else None, built.data_ptr(), _stream_ptr(stream, d)))
    return out_lens, built


# --------------------------------------------------------------------------
# TX pump (tx_resolve -> tx_hold_plan -> tx_solicit_build -> the build of the
# READY frames as one call: two launches for a ring-sized batch).

TX_PUMP_SMALL, TX_PUMP_SMALL_DST = 4096, 4096  # WC_TX_PUMP_SMALL, WC_TX_PUMP_SMALL_DST
TX_PUMP_HELD = 0x80  # WC_TX_PUMP_HELD: the status of a TH_HELD frame, not a TX_* code


class TxPump(NamedTuple):
    """The thirteen outputs of tx_pump, in struct wc_tx_pump_out's order."""
    state: torch.Tensor        # uint8 NR_*, per destination
    miss_list: torch.Tensor    # uint32: NR_MASK_SOLICIT
    miss_count: torch.Tensor   # 1 int64
    hold: torch.Tensor         # uint8 TH_*, per frame
    held_list: torch.Tensor    # uint32: TH_MASK_HELD
    held_count: torch.Tensor   # 1 int64
    sol_lens: torch.Tensor     # uint16, per solicitation slot
    sol_built: torch.Tensor    # 1 int64
    frame_lens: torch.Tensor   # uint16, 0 for a frame that was not built
    status: torch.Tensor       # uint8 TX_*, or TX_PUMP_HELD
    ip_hdr: torch.Tensor       # uint16
    udp: torch.Tensor          # uint16
    errors: torch.Tensor       # 1 int64, accumulated


class _PumpOut(ctypes.Structure):  # struct wc_tx_pump_out
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "state", "miss_list", "miss_count", "hold", "held_list", "held_count", "sol_len",
        "sol_built", "frame_len", "status", "out_ip_hdr", "out_udp", "errors")]


def tx_pump_scratch(n: int, ndst: int) -> int:
    """Bytes of device scratch wc_tx_pump needs for n frames to ndst
    destinations (no GPU)."""
    return int(_lib.active().wc_tx_pump_scratch(int(n), int(ndst)))


def _pump_out(out: Optional[TxPump], n: int, ndst: int, m: int, device) -> TxPump:
    """tx_pump's thirteen tensors: the caller's, checked, or allocated here."""
    if out is None:
        def arr(k, dtype):
            return torch.empty(k, dtype=dtype, device=device)

        def cnt():
            return torch.zeros(1, dtype=torch.int64, device=device)
        return TxPump(arr(ndst, torch.uint8), _index_list(None, ndst, device)[0], cnt(),
                      arr(n, torch.uint8), _index_list(None, n, device)[0], cnt(),
                      arr(m, torch.uint16), cnt(), arr(n, torch.uint16), arr(n, torch.uint8),
                      arr(n, torch.uint16), arr(n, torch.uint16), cnt())
    if not isinstance(out, TxPump):
        raise ValueError("out must be a TxPump (an earlier call's result)")
    _byte_array("state", out.state, ndst, device)
    _byte_array("hold", out.hold, n, device)
    _byte_array("status", out.status, n, device)
    _byte_array("sol_lens", out.sol_lens, m, device, 2)
    for name in ("frame_lens", "ip_hdr", "udp"):
        _byte_array(name, getattr(out, name), n, device, 2)
    _index_list(out.miss_list, ndst, device)
    _index_list(out.held_list, n, device)
    for name in ("miss_count", "held_count", "sol_built", "errors"):
        _byte_array(name, getattr(out, name), 1, device, 8)
    return out


def tx_pump(tab: torch.Tensor, dsts: Optional[torch.Tensor], af: Optional[torch.Tensor],
            descs: torch.Tensor, socks: torch.Tensor, base: torch.Tensor, offsets: torch.Tensor,
            slot_bytes: int, engine: torch.Tensor, sol_out: torch.Tensor,
            sol_offsets: torch.Tensor, sol_slot_bytes: int, zero_udp: bool = False,
            out: Optional[TxPump] = None, scratch: Optional[torch.Tensor] = None, stream=None,
            check: bool = True) -> TxPump:
    """The whole per-batch TX plan and build in one call (wc_tx_pump): every
    output of tx_resolve (``dsts`` / ``af``: the destination table and its
    family bytes, None, None without destinations), tx_hold_plan (``descs`` /
    ``socks``) and tx_solicit_build (``engine``, one solicitation per slot of
    ``sol_offsets`` in ``sol_out``) with their lists, byte for byte, and then the
    build of tx_build_ragged for the ``TH_READY`` frames alone: a ``TH_HELD``
    frame is untouched, has length 0 and status ``TX_PUMP_HELD`` and is not
    counted in ``errors``; a ``TH_MALFORMED`` one is untouched, ``TX_MALFORMED``
    and counted.  Two launches for at most ``TX_PUMP_SMALL`` frames to at most
    ``TX_PUMP_SMALL_DST`` destinations, the chain's calls and the same gated
    build above that; no host round trip in either.  Returns a ``TxPump``; the
    lists hold ``max(n, 1)`` / ``max(ndst, 1)`` entries of which the first
    ``count`` are written.  ``out``: an earlier call's ``TxPump`` to write into
    again (``errors`` is accumulated); ``scratch``: ``tx_pump_scratch(n, ndst)``
    bytes, allocated here unless given -- give both per call in flight when
    ``stream`` is not the current stream.  The caller keeps every frame's slot
    inside ``base``; under ``check`` every solicitation slot is kept inside
    ``sol_out`` and ``sol_out`` off ``base``.  Asynchronous."""
    _same_device(base, offsets=offsets, descs=descs, socks=socks, dsts=dsts, sol_out=sol_out,
                 sol_offsets=sol_offsets)
    d = base.device
    _neigh_tab(tab)
    if tab.device != d:
        raise ValueError(f"tab must be on {d}")
    if not base.is_contiguous() or base.element_size() != 1:
        raise ValueError("base must be a contiguous 1-byte tensor (the frames are written in place)")
    n = offsets.numel()
    if offsets.element_size() != 8 or offsets.is_floating_point() or not offsets.is_contiguous():
        raise ValueError("offsets must be contiguous 8-byte integers")
    if not descs.is_contiguous() or _nbytes(descs) != n * TX_DESC.itemsize:
        raise ValueError("descs must be the contiguous bytes of one TX_DESC per frame")
    ns = _table_tensor("socks", socks, TX_SOCK, TX_BUILD_MAX_SOCKS, d)
    if (dsts is None) != (af is None):
        raise ValueError("dsts and af go together")
    ndst = 0 if dsts is None else _table_tensor("dsts", dsts, TX_DST, _TX_BUILD_MAX_DSTS, d)
    if ndst:
        _byte_array("af", af, ndst, d)
    _engine_tensor(engine, d)
    if not sol_out.is_contiguous() or sol_out.element_size() != 1:
        raise ValueError("sol_out must be a contiguous 1-byte tensor")
    m = sol_offsets.numel()
    if sol_offsets.element_size() != 8 or sol_offsets.is_floating_point() \
            or not sol_offsets.is_contiguous() or m > 0xFFFFFFFF:
        raise ValueError("sol_offsets must be contiguous 8-byte integers, at most 2^32 - 1")
    if not 0 <= int(slot_bytes) <= 0xFFFF or not 0 <= int(sol_slot_bytes) <= 0xFFFF:
        raise ValueError("slot_bytes and sol_slot_bytes are at most 65535")
    if check and m:
        so = sol_offsets.view(torch.int64)
        if bool((so < 0).any()) or int(so.max()) + int(sol_slot_bytes) > _nbytes(sol_out):
            raise ValueError("a solicitation slot [off, off + sol_slot_bytes) runs past sol_out")
        ob, oe = sol_out.data_ptr(), sol_out.data_ptr() + _nbytes(sol_out)
        if ob < base.data_ptr() + _nbytes(base) and base.data_ptr() < oe:
            raise ValueError("sol_out overlaps base: frames and solicitation slots must not overlap")
    o = _pump_out(out, n, ndst, m, d)
    need = tx_pump_scratch(n, ndst)
    if scratch is None:
        scratch = _scratch(need, d)
    elif _nbytes(scratch) < need or scratch.device != d:
        raise ValueError(f"scratch must hold tx_pump_scratch(n, ndst) bytes on {d}")
    c_out = _PumpOut(*[t.data_ptr() or None for t in o])
    with _on_device(d):
        _check("wc_tx_pump", _lib.active().wc_tx_pump(
            tab.data_ptr(), dsts.data_ptr() if ndst else None, af.data_ptr() if ndst else None,
            ndst, descs.data_ptr() if n else None, n, socks.data_ptr() if ns else None, ns,
            base.data_ptr() if n else None, offsets.data_ptr() if n else None, int(slot_bytes),
            _TX_ZERO_UDP_CKSUM if zero_udp else 0, engine.data_ptr(),
            sol_out.data_ptr() if m else None, sol_offsets.data_ptr() if m else None, m,
            int(sol_slot_bytes), ctypes.byref(c_out), scratch.data_ptr(), _stream_ptr(stream, d)))
    return o


def tx_build_host(buf: np.ndarray, offsets: np.ndarray, descs: np.ndarray, socks: np.ndarray,
                  dsts: Optional[np.ndarray], slot_bytes: int,
                  zero_udp: bool = False) -> Tuple[np.ndarray, np.ndarray, int]:
    """tx_build_ragged over host memory (wc_tx_build_host, synchronous): the
    headers are written into ``buf`` in place; (uint16 frame lengths, uint8
    status codes, error count)."""
    flat = _in_place_bytes("tx_build_host", buf)
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    descs = np.ascontiguousarray(descs, dtype=TX_DESC).reshape(-1)
    if descs.size != off.size:
        raise ValueError("one TX_DESC per offset")
    socks = np.ascontiguousarray(socks, dtype=TX_SOCK).reshape(-1)
    dsts = np.zeros(0, TX_DST) if dsts is None else \
        np.ascontiguousarray(dsts, dtype=TX_DST).reshape(-1)
    if socks.size > TX_BUILD_MAX_SOCKS or dsts.size > _TX_BUILD_MAX_DSTS:
        raise ValueError(f"at most {TX_BUILD_MAX_SOCKS} sockets and {_TX_BUILD_MAX_DSTS} "
                         "destinations")
    frame_len = np.empty(off.size, dtype=np.uint16)
    status = np.empty(off.size, dtype=np.uint8)
    errors = ctypes.c_uint64()
    _check("wc_tx_build_host", _lib.active().wc_tx_build_host(
        flat.ctypes.data, flat.size, off.ctypes.data, descs.ctypes.data, off.size,
        socks.ctypes.data if socks.size else None, socks.size,
        dsts.ctypes.data if dsts.size else None, dsts.size, int(slot_bytes),
        _TX_ZERO_UDP_CKSUM if zero_udp else 0, frame_len.ctypes.data, status.ctypes.data,
        ctypes.byref(errors)))
    return frame_len, status, int(errors.value)


# --------------------------------------------------------------------------
# Host-memory batches (end-to-end path).

def cksum_host(buf: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
               kind="ip") -> np.ndarray:
    """Checksum host-resident packets (synchronous), offsets in any order.

    Small batches in a registered buffer are read in place by one kernel;
    larger ones are streamed over pinned H2D copies (wc_cksum_host)."""
    buf, off, lens = _host_batch_args(buf, offsets, lengths)
    out = np.empty(off.size, dtype=np.uint16)
    _check("wc_cksum_host", _lib.active().wc_cksum_host(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, off.size,
        out.ctypes.data, _kind(kind)))
    return out


def _host_batch_args(buf, offsets, lengths):
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    lens_in = np.asarray(lengths)
    if lens_in.size and (lens_in.min() < 0 or lens_in.max() > 0xFFFF):
        raise ValueError("len is a uint16 in the reference (0..65535)")
    offs_in = np.asarray(offsets)
    if offs_in.size and offs_in.dtype.kind == "i" and offs_in.min() < 0:
        raise ValueError("negative offset")
    if offs_in.shape != lens_in.shape:
        raise ValueError("offsets and lengths must have the same shape")
    return (buf, np.ascontiguousarray(offs_in, dtype=np.uint64),
            np.ascontiguousarray(lens_in, dtype=np.uint16))


def cksum_ip_udp_host(buf: np.ndarray, offsets: np.ndarray,
                      lengths: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The fused TX pair over host-memory IP packets (wc_cksum_ip_udp_host,
    synchronous): (IPv4 header checksums -- 0 for IPv6 --, payload_cksum
    results), what mk_ip4_hdr and udp_tx store (ip4.c:184-186,
    udp.c:209-213)."""
    buf, off, lens = _host_batch_args(buf, offsets, lengths)
    hdr = np.empty(off.size, dtype=np.uint16)
    out = np.empty(off.size, dtype=np.uint16)
    _check("wc_cksum_ip_udp_host", _lib.active().wc_cksum_ip_udp_host(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, off.size,
        hdr.ctypes.data, out.ctypes.data))
    return hdr, out


def server_pause() -> None:
    """Stop the resident server grid on every device (wc_server_pause); small
    registered batches take the zero-copy launch until server_resume().  A
    device-wide synchronisation then never waits for the grid."""
    _check("wc_server_pause", _lib.active().wc_server_pause())


def server_resume() -> None:
    _check("wc_server_resume", _lib.active().wc_server_resume())


class server_paused:
    """``with server_paused(): ...`` -- server_pause() / server_resume()."""

    def __enter__(self):
        server_pause()
        return self

    def __exit__(self, *exc):
        server_resume()
        return False


def server_stats() -> dict:
    """The resident server's counters (wc_server_stats): batches served,
    fallbacks to the launch path, grid launches -- process totals."""
    v = [ctypes.c_uint64() for _ in range(3)]
    _check("wc_server_stats", _lib.active().wc_server_stats(*[ctypes.byref(x) for x in v]))
    return dict(zip(("served", "fallbacks", "launches"), (x.value for x in v)))


# Buffers page-locked through host_register, by base address: the library
# pins the pages mapped at that address, so the array is kept alive here until
# host_unregister (a buffer garbage-collected while registered could give its
# address to a new one that the old pinned pages do not back).
_registered: dict = {}


def host_register(buf: np.ndarray) -> None:
    """Page-lock `buf` for the zero-copy / direct-DMA host path.  The array
    is held until host_unregister(buf); registering it (or a new array at the
    same address) again re-pins the pages mapped there now."""
    if not isinstance(buf, np.ndarray) or not buf.flags["C_CONTIGUOUS"]:
        raise ValueError("host_register needs a C-contiguous numpy array")
    _check("wc_host_register", _lib.active().wc_host_register(buf.ctypes.data, buf.nbytes))
    _registered[buf.ctypes.data] = buf


def host_unregister(buf: np.ndarray) -> None:
    addr = buf.ctypes.data
    try:
        _check("wc_host_unregister", _lib.active().wc_host_unregister(addr))
    finally:
        _registered.pop(addr, None)


# --------------------------------------------------------------------------
# Synthetic data / introspection.

def synth_fill(buf: torch.Tensor, seed: int, nbytes: Optional[int] = None,
               stream=None) -> torch.Tensor:
    """Fill a device buffer with the counter-based splitmix64 byte stream."""
    _same_device(buf)
    nbytes = _nbytes(buf) if nbytes is None else nbytes
    if not 0 <= nbytes <= _nbytes(buf):
        raise ValueError(f"nbytes {nbytes} outside the {_nbytes(buf)}-byte buffer")
    with _on_device(buf.device):
        _check("wc_synth_fill", _lib.active().wc_synth_fill(
            _dev_ptr(buf), nbytes, seed & 0xFFFFFFFFFFFFFFFF, _stream_ptr(stream, buf.device)))
    return buf


class SclkProbe:
    """The shader clock beside a timed workload (wc_sclk_probe): one wave on
    a stream of its own samples the 100-MHz wall clock and the shader clock
    counter every `every_us`.  start() before the timed launches (after the
    work before them), mhz() after: the median clock over the samples taken.
    The probe ends by itself after the samples asked for -- keep that inside
    a timed region that ends with a device-wide synchronisation."""

    def __init__(self, device, max_samples: int = 200000):
        self.device = torch.device(device)
        self.max = max_samples
        self.buf = torch.zeros(2 * max_samples, dtype=torch.int64, device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.n = 0

    def start(self, ms: float, every_us: int = 20) -> None:
        self.n = int(min(self.max, max(8, ms * 1e3 / every_us)))
        self.buf.zero_()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with _on_device(self.device):
            _check("wc_sclk_probe", _lib.active().wc_sclk_probe(
                self.buf.data_ptr(), self.n, every_us * 100, self.stream.cuda_stream))

    def mhz(self) -> float:
        self.stream.synchronize()
        s = self.buf[: 2 * self.n].view(self.n, 2).cpu().double()
        dt = s[1:, 0] - s[:-1, 0]
        dc = s[1:, 1] - s[:-1, 1]
        ok = dt > 0
        if not bool(ok.any()):
            return float("nan")
        return float((dc[ok] / dt[ok] * 100.0).median())


def plan_strided(base_addr: int, stride: int, length: int, n: int, kind="ip",
                 fused: bool = False) -> dict:
    """The dispatcher's plan for a strided batch; ``fused``: the plan of
    cksum_ip_udp_strided (``kind`` is then payload's, whatever is given)."""
    vals = [ctypes.c_int() for _ in range(4)]
    refs = [ctypes.byref(v) for v in vals]
    if fused:
        kernel = _lib.active().wc_plan_strided_fused(base_addr, stride, length, n, *refs)
    else:
        _check("wc_plan_strided", _lib.active().wc_plan_strided(
            base_addr, stride, length, n, _kind(kind), *refs))
        kernel = _lib.active().wc_plan_strided_kernel(base_addr, stride, length, n, _kind(kind))
    plan = dict(zip(("group", "chunks_per_lane", "unroll", "grid"), (v.value for v in vals)))
    plan["kernel"] = kernel.decode()
    return plan


def gpu_init(device: int = -1) -> None:
    _check("wc_gpu_init", _lib.active().wc_gpu_init(device))


def version() -> str:
    return _lib.active().wc_version().decode()


# --------------------------------------------------------------------------
# Multi-GPU from one host thread (the C host's path).

def shard_range(n: int, g: int, ngpus: int) -> Tuple[int, int]:
    """The library's even contiguous split: packets [lo, hi) of n for shard g."""
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    _check("wc_shard_range", _lib.active().wc_shard_range(n, g, ngpus, ctypes.byref(lo),
                                                        ctypes.byref(hi)))
    return lo.value, hi.value


_shard_devices: list = []


def gpu_init_multi(ngpus: int = 0, devices=None) -> int:
    """Set up one shard executor per device (devices[g], or g); returns G."""
    global _shard_devices
    arr = None
    if devices is not None:
        devices = [int(d) for d in devices]
        ngpus = len(devices)
        arr = (ctypes.c_int * ngpus)(*devices)
    _check("wc_gpu_init_multi", _lib.active().wc_gpu_init_multi(ngpus, arr))
    G = int(_lib.active().wc_gpu_multi_count())
    _shard_devices = list(devices) if devices is not None else list(range(G))
    return G


def shard_devices() -> list:
    """Device index of every shard executor (after gpu_init_multi)."""
    G = int(_lib.active().wc_gpu_multi_count())
    if len(_shard_devices) != G:
        raise RuntimeError("shard executors not set up by gpu_init_multi")
    return list(_shard_devices)


def cksum_host_multi(buf: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
                     kind="ip") -> np.ndarray:
    """cksum_host split evenly over the shard devices (wc_cksum_host_multi)."""
    buf, off, lens = _host_batch_args(buf, offsets, lengths)
    out = np.empty(off.size, dtype=np.uint16)
    _check("wc_cksum_host_multi", _lib.active().wc_cksum_host_multi(
        buf.ctypes.data, buf.size, off.ctypes.data, lens.ctypes.data, off.size,
        out.ctypes.data, _kind(kind)))
    return out


def _ptrs(ts) -> ctypes.Array:
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if isinstance(t, torch.Tensor) else t
                                         for t in ts])


def _per_shard(name: str, items, devs) -> list:
    """The C side reads one entry per shard executor from every array: each
    list must have exactly that many entries, each on its shard's device."""
    items = list(items)
    if len(items) != len(devs):
        raise ValueError(f"{name}: {len(items)} entries for {len(devs)} shard executors")
    for g, (t, d) in enumerate(zip(items, devs)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name}[{g}] must be a device (cuda) tensor")
        if t.device.index != d:
            raise ValueError(f"{name}[{g}] is on {t.device}, shard {g} runs on cuda:{d}")
    return items


def _shard_streams(streams, devs):
    if streams is None:
        return _ptrs([_stream_ptr(None, torch.device("cuda", d)) for d in devs])
    streams = list(streams)
    if len(streams) != len(devs):
        raise ValueError(f"streams: {len(streams)} entries for {len(devs)} shard executors")
    return _ptrs([_stream_ptr(s, torch.device("cuda", d)) for s, d in zip(streams, devs)])


def cksum_ragged_multi(bases, offsets, lengths, outs, kind="ip", streams=None) -> None:
    """Shard g's device-resident batch (bases[g], offsets[g], lengths[g]) into
    outs[g], each on shard g's device (asynchronous)."""
    k = _kind(kind)
    devs = shard_devices()
    bases = _per_shard("bases", bases, devs)
    offsets = _per_shard("offsets", offsets, devs)
    lengths = _per_shard("lengths", lengths, devs)
    outs = _per_shard("outs", outs, devs)
    for b, o, l, r in zip(bases, offsets, lengths, outs):
        n = _check_ragged(b, o, l, k, True)
        _out_tensor(r, n, b.device)
    ns = (ctypes.c_uint64 * len(devs))(*[o.numel() for o in offsets])
    _check("wc_cksum_ragged_multi", _lib.active().wc_cksum_ragged_multi(
        _ptrs(bases), _ptrs(offsets), _ptrs(lengths), ns, _ptrs(outs), k,
        _shard_streams(streams, devs)))


def gather_results_multi(shard_outs, counts, all_outs, streams=None) -> None:
    """RCCL all-gather of every shard's results into all_outs[g] (packet order)."""
    devs = shard_devices()
    shard_outs = _per_shard("shard_outs", shard_outs, devs)
    all_outs = _per_shard("all_outs", all_outs, devs)
    counts = [int(c) for c in counts]
    if len(counts) != len(devs):
        raise ValueError(f"counts: {len(counts)} entries for {len(devs)} shard executors")
    total = sum(counts)
    for g, (src, c) in enumerate(zip(shard_outs, counts)):
        if c < 0 or src.numel() < c or src.element_size() != 2 or not src.is_contiguous():
            raise ValueError(f"shard_outs[{g}] needs >= {c} contiguous 2-byte entries")
    for g, a in enumerate(all_outs):
        if a.numel() < total or a.element_size() != 2 or not a.is_contiguous():
            raise ValueError("each all_outs tensor needs sum(counts) contiguous 2-byte entries")
    ns = (ctypes.c_uint64 * len(devs))(*counts)
    _check("wc_gather_results_multi", _lib.active().wc_gather_results_multi(
        _ptrs(shard_outs), ns, _ptrs(all_outs), _shard_streams(streams, devs)))
