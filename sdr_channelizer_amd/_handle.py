"""What the Python handle types (Channelizer, Stft) share: the lifecycle of the C handle, the checks a sample buffer
passes before its pointer goes to the library, and the allocation or check of an ``out=`` buffer."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_NP_DTYPE = {L.PFB_FMT_INT8_IQ: np.int8, L.PFB_FMT_INT16_IQ: np.int16, L.PFB_FMT_CF32: np.float32}


def is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class Handle:
    """Base of a class that owns one C handle in ``self._h``.  A subclass sets ``_kind`` (its name in messages) and the
    names of its ``_destroy`` and ``_get_device`` entry points, sets ``self.fmt`` and calls ``_created`` once the
    library has made the handle."""

    _kind = "handle"
    _destroy = ""
    _get_device = ""

    def _created(self, lib) -> None:
        self._lib = lib
        dev = C.c_int(-1)  # device=-1: the library took the device current at creation; it says which one that was
        L.check(getattr(lib, self._get_device)(self._h, C.byref(dev)), self._get_device)
        self._device_index = int(dev.value)

    @property
    def device_index(self) -> int:
        """The HIP device ordinal the handle lives on (device=-1 at construction = the device current at that moment)."""
        return self._device_index

    # -- lifecycle ---------------------------------------------------------------
    def release(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def close(self) -> None:
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    # -- samples -----------------------------------------------------------------
    def _host_samples(self, iq) -> tuple[np.ndarray, int]:
        want = _NP_DTYPE[self.fmt]
        a = np.asarray(iq)
        if self.fmt == L.PFB_FMT_CF32 and np.iscomplexobj(a):
            a = np.ascontiguousarray(a, dtype=np.complex64).view(np.float32)
        if a.dtype != want:
            raise TypeError(f"expected {np.dtype(want)} I/Q for this {self._kind}, got {a.dtype}")
        a = np.ascontiguousarray(a).reshape(-1)
        if a.size % 2:
            raise ValueError("interleaved I,Q needs an even element count")
        return a, a.size // 2

    def _device_samples(self, iq) -> int:
        """Validate a CUDA tensor of raw samples against the handle (dtype, device, contiguity) BEFORE its pointer goes
        to the library -- a wrong dtype would be read at the handle's sample size, past the end of the allocation --
        and return its length in complex samples."""
        import torch
        want = {L.PFB_FMT_INT8_IQ: (torch.int8,), L.PFB_FMT_INT16_IQ: (torch.int16,),
                L.PFB_FMT_CF32: (torch.float32, torch.complex64)}[self.fmt]
        if iq.dtype not in want:
            raise TypeError(f"expected {want[0]} I/Q for this {self._kind}, got {iq.dtype}")
        dev = self.device_index
        if iq.device.index != dev:
            raise ValueError(f"I/Q tensor is on cuda:{iq.device.index}, the {self._kind} on cuda:{dev}")
        if not iq.is_contiguous():
            raise ValueError("device I/Q must be contiguous")
        if iq.is_complex():
            return iq.numel()
        if iq.numel() % 2 or (iq.dim() >= 2 and iq.shape[-1] != 2):
            raise ValueError("interleaved I,Q: the last dimension must be 2 (or a flat tensor of even length)")
        return iq.numel() // 2

    @staticmethod
    def _output(out, shape: tuple[int, int], complex_out: bool, device=None):
        """Allocate the output of a call, or check the caller's ``out`` before the library writes prod(shape) values
        through its pointer; returned viewed as ``shape``.  ``device``: the torch device of a CUDA output, None for a
        numpy one."""
        count = shape[0] * shape[1]
        if device is None:
            dt = np.dtype(np.complex64 if complex_out else np.float32)
            if out is None:
                return np.empty(shape, dtype=dt)
            if not isinstance(out, np.ndarray) or out.dtype != dt or out.size < count or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {dt} numpy array with room for {count} values")
        else:
            import torch
            dt = torch.complex64 if complex_out else torch.float32
            if out is None:
                return torch.empty(shape, dtype=dt, device=device)
            if (not is_torch(out) or not out.is_cuda or out.device != device or out.numel() < count or out.dtype != dt
                    or not out.is_contiguous()):
                raise ValueError(f"out must be a contiguous {dt} tensor on {device} with room for {count} values")
        return out if tuple(out.shape) == shape else out.reshape(-1)[:count].reshape(shape)
