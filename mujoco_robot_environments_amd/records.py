"""Episode-record encoding on the device: torch-facing wrappers of ``mre_varint_pack_rows`` / ``mre_crc32c_rows``
(include/mre.h, csrc/mre_records.hip) -- the packed varints TFDS stores a uint8 image as, and the CRC-32C that TFRecord
framing wants, computed where the rendered frames already are.  Everything is enqueued on torch's current stream;
nothing here synchronises.  ``dataset.BatchedEpisodeLogger`` is the user.
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
