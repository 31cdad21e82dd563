"""Wake windows (ocean_wake, include/oceanfft.h): a square height field in base-point space, forced by the
vertical loads of hull points and stepped on the device with the 13 x 13 deep-water operator."""
from __future__ import annotations

import ctypes

import numpy as np

from .capi import OceanWakeSettings, check, lib
from .hip import DeviceBuffer, to_host

__all__ = ["Wake", "default_wake_settings", "apply_wake_settings"]

_INT_FIELDS = ("substeps", "border")
_FIELDS = ("dt", "substeps", "gravity", "rho_g", "damp", "edge_damp", "border")


def default_wake_settings(**overrides) -> OceanWakeSettings:
    """ocean_wake_settings defaults (1/60 s in 4 substeps, 9.8, 9810, damp 0.05, edge_damp 8, border 16) with
    keyword overrides."""
    s = OceanWakeSettings()
    lib().ocean_default_wake_settings(ctypes.byref(s))
    return apply_wake_settings(s, **overrides)


def apply_wake_settings(s: OceanWakeSettings, **overrides) -> OceanWakeSettings:
    for k, v in overrides.items():
        if k not in _FIELDS:
            raise AttributeError(f"ocean_wake_settings has no field {k!r}")
        setattr(s, k, int(v) if k in _INT_FIELDS else float(v))
    return s


class Wake:
    """One window of size x size texels of dx metres on the plan `fft`; texel (0, 0) at (origin_x, origin_z).
    With fft=None the window has no device storage (ocean_debug_wake_create_host): taps, bound and argument
    checks only."""

    def __init__(self, fft, size: int, dx: float, origin_x: float = 0.0, origin_z: float = 0.0, smoothing: float = 0.0):
        h = ctypes.c_void_p()
        if fft is None:
            check(lib().ocean_debug_wake_create_host(ctypes.byref(h), int(size), dx, origin_x, origin_z, smoothing),
                  "ocean_debug_wake_create_host")
        else:
            check(lib().ocean_wake_create(ctypes.byref(h), fft.handle, int(size), dx, origin_x, origin_z, smoothing),
                  "ocean_wake_create")
        self._h = h
        self.fft = fft
        self.size = int(lib().ocean_wake_size(h))
        self.dx = float(np.float32(dx))

    @property
    def handle(self):
        return self._h

    def kernel(self) -> np.ndarray:
        """The (7, 7) float32 taps T[a][b] as the device uses them."""
        out = np.zeros(49, np.float32)
        check(lib().ocean_wake_kernel(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), "ocean_wake_kernel")
        return out.reshape(7, 7)

    def max_substep(self, gravity: float = 9.8) -> float:
        return float(lib().ocean_wake_max_substep(self._h, gravity))

    def origin(self):
        """(ox, oz): the base point of texel (0, 0) after the shifts so far."""
        out = (ctypes.c_float * 2)()
        check(lib().ocean_wake_origin(self._h, out), "ocean_wake_origin")
        return float(out[0]), float(out[1])

    def height_ptr(self) -> int:
        """The device address of the current h; it changes with ocean_wake_step."""
        return int(lib().ocean_wake_height(self._h) or 0)

    def height_host(self) -> np.ndarray:
        """(size, size) float32, [j][i]; synchronises the plan's stream."""
        self.fft.synchronize()
        return to_host(self.height_ptr(), (self.size, self.size))

    def height(self):
        """The current h as a torch view (size, size) of the device memory, [j][i]: no copy. Valid until the
        next step; the caller orders its own stream against the plan's."""
        import torch

        class _Span:
            pass

        span = _Span()
        span.__cuda_array_interface__ = {"shape": (self.size, self.size), "typestr": "<f4",
                                         "data": (self.height_ptr(), False), "version": 2}
        span.owner = self  # the window outlives the view
        return torch.as_tensor(span, device="cuda")

    def reset(self) -> None:
        check(lib().ocean_wake_reset(self._h), "ocean_wake_reset")

    def shift(self, di: int, dj: int) -> None:
        check(lib().ocean_wake_shift(self._h, int(di), int(dj)), "ocean_wake_shift")

    def step_ptr(self, records_ptr: int = 0, max_records: int = 0, count_ptr: int = 0,
                 settings: OceanWakeSettings = None, **overrides) -> None:
        """Enqueue one ocean_wake_step: records at a device pointer (rows of 8 floats, the layout of the hulls'
        point_out), their count at a device int64 (0: max_records)."""
        if settings is None:
            settings = default_wake_settings(**overrides)
        elif overrides:
            raise TypeError("Wake.step: pass settings or their fields, not both")
        check(lib().ocean_wake_step(self._h, ctypes.byref(settings), ctypes.c_void_p(records_ptr),
                                    ctypes.c_void_p(count_ptr), ctypes.c_int64(max_records)), "ocean_wake_step")

    def step(self, records=None, settings: OceanWakeSettings = None, **overrides) -> None:
        """Enqueue one ocean_wake_step from a float32 CUDA tensor of shape (n, 8), or None for a free step. The
        tensor must be ready in the plan's stream order and stay alive until the step has run."""
        if records is None:
            return self.step_ptr(0, 0, 0, settings, **overrides)
        import torch

        if not (records.is_cuda and records.is_contiguous() and records.dtype == torch.float32 and records.dim() == 2
                and records.shape[1] == 8):
            raise TypeError("Wake.step: records must be a contiguous float32 CUDA tensor of shape (n, 8)")
        self.step_ptr(records.data_ptr() if records.shape[0] else 0, int(records.shape[0]), 0, settings, **overrides)

    def step_host(self, records: np.ndarray = None, count: int = None, settings: OceanWakeSettings = None,
                  **overrides) -> np.ndarray:
        """One step from host records (n, 8), of which a device count `count` (None: all) are used; returns h."""
        rec = cnt = None
        n = 0
        if records is not None:
            records = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
            n = records.shape[0]
            rec = DeviceBuffer.from_array(records) if n else None
            if count is not None:
                cnt = DeviceBuffer.from_array(np.array([count], np.int64))
        self.step_ptr(rec.ptr if rec else 0, n, cnt.ptr if cnt else 0, settings, **overrides)
        return self.height_host()

    def sample_ptr(self, xz_ptr: int, n: int, out_ptr: int) -> None:
        check(lib().ocean_wake_sample(self._h, ctypes.c_void_p(xz_ptr), ctypes.c_int64(n), ctypes.c_void_p(out_ptr)),
              "ocean_wake_sample")

    def sample_host(self, xz: np.ndarray) -> np.ndarray:
        """(n, 4) float32 (h, dh/dx, dh/dz, dh/dt) at host base points (n, 2)."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        n = xz.shape[0]
        src = DeviceBuffer.from_array(xz) if n else None
        out = DeviceBuffer(max(n, 1) * 16)
        self.sample_ptr(src.ptr if src else 0, n, out.ptr)
        self.fft.synchronize()
        return out.to_host((n, 4))

    def close(self) -> None:
        if self._h:
            lib().ocean_wake_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
