"""Episode-record encoding on the device: torch-facing wrappers of ``mre_varint_pack_rows`` / ``mre_crc32c_rows``
(include/mre.h, csrc/mre_records.hip) -- the packed varints TFDS stores a uint8 image as, and the CRC-32C that TFRecord
framing wants, computed where the rendered frames already are -- and of ``mre_varint_unpack_rows``, which turns a
shard's packed lists back into frames.  Everything is enqueued on torch's current stream; nothing here synchronises.
``dataset.BatchedEpisodeLogger`` and ``dataset.read_episodes_device`` are the users.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import lib as _lib


def _rows(src: torch.Tensor):
    """(pointer, row stride in bytes, bytes per row, source rows) of a CUDA tensor whose rows (dim 0) are contiguous."""
    if not src.is_cuda or src.dim() < 1 or src.shape[0] < 1:
        raise ValueError("rows must be a non-empty CUDA tensor")
    if not src[0].is_contiguous():
        raise ValueError("every row (index along dim 0) must be contiguous")
    es = src.element_size()
    stride = src.stride(0) * es if src.dim() > 1 else es
    return src.data_ptr(), int(stride), int(src[0].numel() * es), int(src.shape[0])


def row_index(idx, src_rows: int, device) -> torch.Tensor:
    """Index list for the calls below: int32 on the device, every entry checked against the source on the host."""
    a = np.ascontiguousarray(idx, np.int64).reshape(-1)
    if a.size == 0 or a.min() < 0 or a.max() >= src_rows:
        raise ValueError(f"row index list empty or outside 0..{src_rows - 1}")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def _call(src: torch.Tensor, idx: Optional[torch.Tensor]):
    ptr, stride, row_bytes, src_rows = _rows(src)
    if idx is not None:
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous()):
            raise ValueError("idx must be a contiguous int32 CUDA vector (row_index())")
    rows = src_rows if idx is None else int(idx.numel())
    L = _lib.lib()
    ws_bytes = int(L.mre_records_workspace_bytes(rows, row_bytes))
    if ws_bytes == 0:
        raise ValueError(f"rows of {row_bytes} bytes are not supported")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=src.device)
    stream = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    head = (stream, ptr, stride, row_bytes, None if idx is None else idx.data_ptr(), src_rows, rows)
    return L, head, rows, row_bytes, ws, ws_bytes


def varint_size_rows(src: torch.Tensor, idx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(off int64 [R], len int32 [R]) of the packed varints of every selected row, without packing them."""
    L, head, rows, _, ws, ws_bytes = _call(src, idx)
    off = torch.empty(rows, dtype=torch.int64, device=src.device)
    ln = torch.empty(rows, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(L.mre_varint_pack_rows(*head, None, 0, off.data_ptr(), ln.data_ptr(), None, ws.data_ptr(), ws_bytes),
                   "mre_varint_pack_rows")
    return off, ln


def varint_pack_rows(src: torch.Tensor, idx: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """Packed varints of every selected row of a uint8 CUDA tensor: (out uint8, off int64 [R], len int32 [R],
    crc int32 [R]; view the last two as uint32).  ``out`` (uint8 CUDA, at least 2 * R * row_bytes) is allocated when
    not given; row r occupies out[off[r] : off[r] + len[r]]."""
    if src.dtype != torch.uint8:
        raise ValueError("varints are packed from uint8 rows")
    L, head, rows, row_bytes, ws, ws_bytes = _call(src, idx)
    if out is None:
        out = torch.empty(2 * rows * row_bytes, dtype=torch.uint8, device=src.device)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 CUDA tensor")
    off = torch.empty(rows, dtype=torch.int64, device=src.device)
    ln = torch.empty(rows, dtype=torch.int32, device=src.device)
    crc = torch.empty(rows, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(L.mre_varint_pack_rows(*head, out.data_ptr(), int(out.numel()), off.data_ptr(), ln.data_ptr(),
                                          crc.data_ptr(), ws.data_ptr(), ws_bytes), "mre_varint_pack_rows")
    return out, off, ln, crc


def crc32c_rows(src: torch.Tensor, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CRC-32C of the bytes of every selected row of a CUDA tensor (any dtype): int32 [R], view as uint32."""
    L, head, rows, _, ws, ws_bytes = _call(src, idx)
    crc = torch.empty(rows, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(L.mre_crc32c_rows(*head, crc.data_ptr(), ws.data_ptr(), ws_bytes), "mre_crc32c_rows")
    return crc


def _descriptor(x, rows: Optional[int], device, what: str):
    """(device int64 [rows] tensor, host int64 array or None) of one descriptor given as a CUDA tensor or as host data."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if not (x.dtype == torch.int64 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous int64 vector")
        host = None
    else:
        host = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x)
        if host.dtype.kind not in "iu" or host.ndim != 1:
            raise ValueError(f"{what} must be a vector of integers")
        host = host.astype(np.int64)
        x = torch.from_numpy(host).to(device, non_blocking=True)
    if rows is not None and int(x.numel()) != rows:
        raise ValueError(f"{what} has {int(x.numel())} entries, {rows} rows are described")
    return x, host


def varint_unpack_rows(src: torch.Tensor, src_off, src_len, nvalues, out_off, max_src_len: Optional[int] = None,
                       out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """The inverse of ``varint_pack_rows`` for rows as a shard holds them: row r is the packed bytes
    src[src_off[r] : src_off[r] + src_len[r]] of a uint8 CUDA buffer (a file's bytes), and its nvalues[r] values go to
    out[out_off[r] : out_off[r] + nvalues[r]] as uint8.  Returns (out uint8, status int32 [R]): status[r] is 0 or a
    set of lib.MRE_UNPACK_* bits (malformed bytes or a descriptor outside the buffers are flagged, never followed;
    include/mre.h).  The descriptors are int64 vectors, on the device or on the host (host ones are uploaded);
    ``max_src_len`` (the largest src_len) and the size of ``out`` are taken from host descriptors when not given, and
    must be given with device ones -- nothing here reads the device back."""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous() and src.numel() > 0):
        raise ValueError("src must be a non-empty contiguous uint8 CUDA vector")
    dev = src.device
    d_so, h_so = _descriptor(src_off, None, dev, "src_off")
    rows = int(d_so.numel())
    if rows < 1:
        raise ValueError("no rows are described")
    d_sl, h_sl = _descriptor(src_len, rows, dev, "src_len")
    d_nv, h_nv = _descriptor(nvalues, rows, dev, "nvalues")
    d_oo, h_oo = _descriptor(out_off, rows, dev, "out_off")
    for d in (d_so, d_sl, d_nv, d_oo):
        if d.device != dev:
            raise ValueError("the descriptors must be on src's device")
    if max_src_len is None:
        if h_sl is None:
            raise ValueError("max_src_len must be given when src_len is on the device")
        max_src_len = max(1, int(h_sl.max()))
    if out is None:
        if h_nv is None or h_oo is None:
            raise ValueError("out must be given when nvalues / out_off are on the device")
        out = torch.empty(max(1, int((h_oo + h_nv).max())), dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev):
        raise ValueError("out must be a contiguous uint8 CUDA tensor on src's device")
    if status is None:
        status = torch.empty(rows, dtype=torch.int32, device=dev)
    if not (status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == rows
            and status.device == dev):
        raise ValueError("status must be a contiguous int32 CUDA vector with one entry per row")
    L = _lib.lib()
    ws_bytes = int(L.mre_varint_unpack_workspace_bytes(rows, int(max_src_len)))
    if ws_bytes == 0:
        raise ValueError(f"rows of up to {max_src_len} packed bytes are not supported")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.mre_varint_unpack_rows(stream, src.data_ptr(), int(src.numel()), d_so.data_ptr(), d_sl.data_ptr(),
                                            d_nv.data_ptr(), d_oo.data_ptr(), rows, int(max_src_len), out.data_ptr(),
                                            int(out.numel()), status.data_ptr(), ws.data_ptr(), ws_bytes),
                   "mre_varint_unpack_rows")
    return out, status
