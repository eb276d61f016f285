"""Where the buffers of one library call live, and everything a binding needs to know about that.

A binding asks this module where its buffers live -- `place_of` its inputs gives the host or one torch device -- and takes
allocation (`Place.new`), pointers (`Place.addr`, `Place.addr_or_null`), the wait for torch's producers (`Place.sync`) and the
int32 -> int64 index conversion (`Place.index64`) from that place; it never branches on torch itself for any of them.  The
input checks that several bindings share are here too.  torch is imported only where a device tensor has shown up.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi


def is_device_tensor(a):
    return a is not None and hasattr(a, "data_ptr") and bool(getattr(a, "is_cuda", False))


# numpy type -> name of the torch dtype of a buffer on the device; uint32 words are an int32 tensor holding their bits
_TORCH_DTYPE = {np.float64: "float64", np.float32: "float32", np.int64: "int64", np.int32: "int32", np.uint32: "int32", np.uint8: "uint8",
                np.bool_: "bool"}


class Place:
    """The host (``device`` None) or one torch device: where the buffers of one library call live."""

    def __init__(self, device=None):
        self.device = device
        self.mem = _ffi.AI_MEM_HOST if device is None else _ffi.AI_MEM_DEVICE
        if device is not None:   # torch is imported only once a device tensor has shown up
            import torch
            self._torch = torch
            self._dtypes = {np_type: getattr(torch, name) for np_type, name in _TORCH_DTYPE.items()}

    def dtype(self, np_type):
        """A numpy type (``np.float64``, ...) as this place spells it: itself on the host, the torch dtype of the table on the device."""
        return np_type if self.device is None else self._dtypes[np_type]

    def new(self, shape, np_type):
        """An uninitialised buffer of ``shape``."""
        if self.device is None:
            return np.empty(shape, dtype=np_type)
        return self._torch.empty(shape, dtype=self._dtypes[np_type], device=self.device)

    def zeros(self, shape, np_type):
        if self.device is None:
            return np.zeros(shape, dtype=np_type)
        return self._torch.zeros(shape, dtype=self._dtypes[np_type], device=self.device)

    def addr(self, a):
        """The pointer of a buffer of this place as a library call takes it; None (NULL, "not given" / "not wanted") for None."""
        if a is None:
            return None
        return a.ctypes.data if self.device is None else C.c_void_p(a.data_ptr())

    def addr_or_null(self, a):
        """`addr`, but NULL for a buffer without elements too: for the arguments whose entry takes "nothing there" as NULL."""
        return self.addr(a) if a is not None and (a.size if self.device is None else a.numel()) else None

    def index64(self, a):
        """An int32 result of this place as int64 indices, where it lives."""
        return a.astype(np.int64) if self.device is None else a.long()

    def sync(self):
        """Wait for what torch has queued on its current stream of the device (concatenations, copies, uploads, the caller's own
        producers): the library reads on its own stream.  Stands directly before the library call; nothing to do on the host."""
        if self.device is not None:
            self._torch.cuda.current_stream(self.device).synchronize()


HOST = Place()


def place_of(*arrays):
    """The place of the first device tensor among ``arrays``, or the host when there is none."""
    for a in arrays:
        if is_device_tensor(a):
            return Place(a.device)
    return HOST


def grow(call, cap):
    """``(total, result)`` of ``call(cap)``, asked again with the reported total as the capacity while that exceeds ``cap``."""
    while True:
        total, result = call(cap)
        if total <= cap:
            return total, result
        cap = int(total)


def points_f64(a, name="points"):
    """(n, 3) float64 contiguous array or device tensor; an object with ``.points`` (an open3d cloud) gives its points."""
    if is_device_tensor(a):
        import torch
        if a.dtype != torch.float64 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} on the device must be a float64 (n, 3) tensor")
        return a.contiguous()
    if not isinstance(a, np.ndarray) and hasattr(a, "points"):
        a = a.points
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size == 0:
        a = a.reshape(0, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must be (n, 3)")
    return a


def rows(a, cols, dtype, name, place):
    """One contiguous (n, cols) array (host) or tensor (device) of ``dtype``; ``cols`` None: any width."""
    if place.device is not None:
        want = place.dtype(dtype)
        if not is_device_tensor(a) or a.dtype != want or a.dim() != 2 or (cols is not None and a.shape[1] != cols):
            raise ValueError(f"{name} on the device must be {want} (n, {cols or 'F'}) tensors")
        return a.contiguous()
    a = np.asarray(a)
    if a.size == 0 and a.ndim != 2:
        a = a.reshape(0, cols or 0)
    if a.ndim != 2 or (cols is not None and a.shape[1] != cols):
        raise ValueError(f"{name} must be (n, {cols or 'F'}) arrays")
    return np.ascontiguousarray(a, dtype=dtype)


def offsets_of(lengths):
    """int64 offsets (len(lengths) + 1 entries, from 0) of segments of these lengths."""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
    return off


def concat(parts, cols, dtype, name, place):
    """(all rows, int64 offsets with len(parts) + 1 entries) of a list of per-segment (n_s, cols) arrays or tensors.  Segments
    without rows only count in the offsets; with no row at all the result is (0, width of the first part, or 0)."""
    if not isinstance(parts, (list, tuple)):
        raise ValueError(f"{name}: a list of per-segment arrays, or one array together with its offsets, is expected")
    seq = [rows(a, cols, dtype, name, place) for a in parts]
    off = offsets_of([int(a.shape[0]) for a in seq])
    full = [a for a in seq if a.shape[0]]
    if len({int(a.shape[1]) for a in full}) > 1:
        raise ValueError(f"{name}: every segment must have the same width")
    if not full:
        return place.zeros((0, int(seq[0].shape[1]) if seq else (cols or 0)), dtype), off
    if place.device is not None:
        import torch
        return torch.cat(full), off
    return np.concatenate(full), off


def segmented(parts, offsets, cols, dtype, name, place):
    """`concat` of a list, or the caller's own concatenated array with its offsets."""
    if offsets is None:
        return concat(parts, cols, dtype, name, place)
    return rows(parts, cols, dtype, name, place), np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)


def cat_int32(parts, place):
    """Flat per-segment integer ids (host arrays or device tensors, the caller has checked them) as one int32 buffer at `place`."""
    if place.device is not None:
        import torch
        parts = [a.to(device=place.device, dtype=torch.int32) if is_device_tensor(a) else
                 torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=place.device) for a in parts]
        return torch.cat(parts).contiguous() if parts else place.zeros(0, np.int32)
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.int32) if parts else np.zeros(0, dtype=np.int32)
