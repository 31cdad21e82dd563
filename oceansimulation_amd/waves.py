"""Python mirror of the reference's Waves::FFTCalculator / Waves::Generator over the C ABI.

Same names and argument meaning as src/FFTCalculator.h:11-59 and src/Generator.h:33-93 (snake_case
aliases added); errors raise OceanError (the reference has no error path). Outputs are device
pointers into HBM owned by the objects; `*_host()` helpers copy them out for checking.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi, hip
from .capi import (OceanFoamDepositSettings, OceanFoamSettings, OceanParticleSettings, OceanSettings, OceanSpraySettings,
                   check, lib)


def default_settings(**overrides) -> OceanSettings:
    """GeneratorSettings defaults (src/Generator.h:14-29) with keyword overrides."""
    s = OceanSettings()
    lib().ocean_default_settings(ctypes.byref(s))
    apply_settings(s, **overrides)
    return s


def apply_settings(s: OceanSettings, **overrides) -> OceanSettings:
    for k, v in overrides.items():
        if k == "seed":
            s.seed[0], s.seed[1] = int(v[0]), int(v[1])
        else:
            setattr(s, k, v)
    return s


def default_foam_settings(**overrides) -> OceanFoamSettings:
    """ocean_foam_settings defaults (bias 0.9, gain 8, decay 0.5, level 0.5) with keyword overrides."""
    s = OceanFoamSettings()
    lib().ocean_default_foam_settings(ctypes.byref(s))
    return apply_foam_settings(s, **overrides)


def apply_foam_settings(s: OceanFoamSettings, **overrides) -> OceanFoamSettings:
    for k, v in overrides.items():
        if k not in ("bias", "gain", "decay", "level"):
            raise AttributeError(f"ocean_foam_settings has no field {k!r}")
        setattr(s, k, v)
    return s


def default_foam_deposit_settings(**overrides) -> OceanFoamDepositSettings:
    """ocean_foam_deposit_settings defaults (amount 0.05, per_speed 0.01) with keyword overrides."""
    s = OceanFoamDepositSettings()
    lib().ocean_default_foam_deposit_settings(ctypes.byref(s))
    return apply_foam_deposit_settings(s, **overrides)


def apply_foam_deposit_settings(s: OceanFoamDepositSettings, **overrides) -> OceanFoamDepositSettings:
    for k, v in overrides.items():
        if k not in ("amount", "per_speed"):
            raise AttributeError(f"ocean_foam_deposit_settings has no field {k!r}")
        setattr(s, k, v)
    return s


def default_spray_settings(**overrides) -> OceanSpraySettings:
    """ocean_spray_settings defaults (threshold 0.9, rate 8, seed 0) with keyword overrides."""
    s = OceanSpraySettings()
    lib().ocean_default_spray_settings(ctypes.byref(s))
    return apply_spray_settings(s, **overrides)


def apply_spray_settings(s: OceanSpraySettings, **overrides) -> OceanSpraySettings:
    for k, v in overrides.items():
        if k not in ("threshold", "rate", "seed"):
            raise AttributeError(f"ocean_spray_settings has no field {k!r}")
        setattr(s, k, v)
    return s


def default_particle_settings(**overrides) -> OceanParticleSettings:
    """ocean_particle_settings defaults (gravity 9.8, drag 0.5, no wind, lifetime 4, gain 1, lift 10, 4
    iterations, tolerance 1e-3) with keyword overrides."""
    s = OceanParticleSettings()
    lib().ocean_default_particle_settings(ctypes.byref(s))
    return apply_particle_settings(s, **overrides)


def apply_particle_settings(s: OceanParticleSettings, **overrides) -> OceanParticleSettings:
    names = [f[0] for f in OceanParticleSettings._fields_]
    for k, v in overrides.items():
        if k not in names:
            raise AttributeError(f"ocean_particle_settings has no field {k!r}")
        if k == "wind":
            s.wind[0], s.wind[1], s.wind[2] = float(v[0]), float(v[1]), float(v[2])
        else:
            setattr(s, k, v)
    return s


class FFTCalculator:
    """Waves::FFTCalculator (src/FFTCalculator.h:11-59)."""

    def __init__(self, texture_size: int = 512, stream: int | None = None):
        h = ctypes.c_void_p()
        check(lib().ocean_fft_create(ctypes.byref(h), texture_size, ctypes.c_void_p(stream or 0)),
              "ocean_fft_create")
        self._h = h
        self.texture_size = texture_size

    def GetTextureResolution(self) -> int:
        return int(lib().ocean_fft_texture_resolution(self._h))

    get_texture_resolution = GetTextureResolution

    def EncodeIFFT(self, image_ptr: int) -> None:
        """In-place iFFT of a device RGBA32F N x N image (src/FFTCalculator.cpp:73-114)."""
        check(lib().ocean_fft_encode_ifft(self._h, ctypes.c_void_p(image_ptr)), "ocean_fft_encode_ifft")

    encode_ifft = EncodeIFFT

    def encode_ifft_batch(self, images_ptr: int, n_images: int) -> None:
        check(lib().ocean_fft_encode_ifft_batch(self._h, ctypes.c_void_p(images_ptr), n_images),
              "ocean_fft_encode_ifft_batch")

    def synchronize(self) -> None:
        check(lib().ocean_fft_synchronize(self._h), "ocean_fft_synchronize")

    @property
    def cus(self) -> int:
        return int(lib().ocean_fft_device_cus(self._h))

    def set_cu_budget(self, cus: int) -> None:
        """Size this plan's persistent grids for `cus` CUs (0 = all); see ocean_fft_set_cu_budget."""
        check(lib().ocean_fft_set_cu_budget(self._h, int(cus)), "ocean_fft_set_cu_budget")

    def debug_work_limit(self, nbytes: int | None) -> None:
        """Cap EncodeIFFT's work image / slab at `nbytes` (None: no cap); 0 forces the in-place passes.
        See ocean_debug_fft_work_limit."""
        cap = ctypes.c_size_t(-1).value if nbytes is None else int(nbytes)
        check(lib().ocean_debug_fft_work_limit(self._h, cap), "ocean_debug_fft_work_limit")

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h:
            lib().ocean_fft_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Generator:
    """Waves::Generator (src/Generator.h:33-93), batched over `cascades` cascades sharing N."""

    def __init__(self, fft: FFTCalculator, cascades: int = 1):
        h = ctypes.c_void_p()
        check(lib().ocean_generator_create(ctypes.byref(h), fft.handle, cascades), "ocean_generator_create")
        self._h = h
        self.fft = fft
        self.n = fft.GetTextureResolution()
        self.cascades = cascades

    @property
    def handle(self):
        return self._h

    def set_half_spectrum(self, enable: bool) -> None:
        """Select the half-spectrum (default where supported) or the full-spectrum frame path."""
        check(lib().ocean_generator_set_half_spectrum(self._h, 1 if enable else 0), "ocean_generator_set_half_spectrum")

    def set_four_step(self, enable: bool) -> None:
        """Whole grids of 8192 / 16384 on one rank: the four-step column pass (default) or the
        strip-dealt column pass + transposes that multi-rank slabs run (bit-identical to them)."""
        check(lib().ocean_generator_set_four_step(self._h, 1 if enable else 0), "ocean_generator_set_four_step")

    def set_h0_memo(self, enable: bool) -> None:
        """Skip requested re-seeds whose h0 inputs are unchanged (default) or re-seed every time."""
        check(lib().ocean_generator_set_h0_memo(self._h, 1 if enable else 0), "ocean_generator_set_h0_memo")

    def set_frame_overlap(self, enable: bool) -> None:
        """Run frame f + 1's column pass beside frame f's row pass (whole grids of 1024..4096, half
        spectrum; bit-identical results; pays at 1-2 cascades)."""
        check(lib().ocean_generator_set_frame_overlap(self._h, 1 if enable else 0),
              "ocean_generator_set_frame_overlap")

    def frame_bytes(self):
        """Algorithmic HBM bytes per point of the column and row pass of the current path."""
        out = (ctypes.c_double * 2)()
        check(lib().ocean_generator_frame_bytes(self._h, out), "ocean_generator_frame_bytes")
        return float(out[0]), float(out[1])

    def GetOceanSettings(self, cascade: int = 0) -> OceanSettings:
        p = lib().ocean_generator_settings(self._h, cascade)
        if not p:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_settings")
        return p.contents

    get_ocean_settings = GetOceanSettings

    def CalculateOcean(self, timestep: float, update_ocean: bool = False) -> None:
        check(lib().ocean_generator_calculate(self._h, ctypes.c_float(timestep), 1 if update_ocean else 0),
              "ocean_generator_calculate")

    calculate_ocean = CalculateOcean

    def GenerateSpectrum(self) -> None:
        check(lib().ocean_generator_generate_spectrum(self._h), "ocean_generator_generate_spectrum")

    def GetHeightMap(self, cascade: int = 0) -> int:
        return int(lib().ocean_generator_height_map(self._h, cascade))

    def GetDisplacementMap(self, cascade: int = 0) -> int:
        return int(lib().ocean_generator_displacement_map(self._h, cascade))

    def GetJacobianMap(self, cascade: int = 0) -> int:
        return int(lib().ocean_generator_jacobian_map(self._h, cascade))

    def GetInitialSpectrum(self, cascade: int = 0) -> int:
        return int(lib().ocean_generator_initial_spectrum(self._h, cascade))

    # ---- host copies (checking / export) ----
    def height_map_host(self, cascade: int = 0) -> np.ndarray:
        self.fft.synchronize()
        return hip.to_host(self.GetHeightMap(cascade), (self.n, self.n, 4))

    def displacement_map_host(self, cascade: int = 0) -> np.ndarray:
        self.fft.synchronize()
        return hip.to_host(self.GetDisplacementMap(cascade), (self.n, self.n, 4))

    def jacobian_map_host(self, cascade: int = 0) -> np.ndarray:
        self.fft.synchronize()
        return hip.to_host(self.GetJacobianMap(cascade), (self.n, self.n))

    def initial_spectrum_host(self, cascade: int = 0) -> np.ndarray:
        """h0 as an N x N x 4 row-major image (de-blocked from the device's strip-blocked layout)."""
        self.fft.synchronize()
        b = int(lib().ocean_generator_spectrum_block(self._h))
        blocked = hip.to_host(self.GetInitialSpectrum(cascade), (self.n // b, self.n, b, 4))
        return np.ascontiguousarray(blocked.transpose(1, 0, 2, 3).reshape(self.n, self.n, 4))

    # ---- mip pyramid of the maps (ocean_generator_build_mips, include/oceanfft.h) ----
    def build_mips(self) -> None:
        """Enqueue the rebuild of levels >= 1 of every cascade's three maps from the current maps."""
        check(lib().ocean_generator_build_mips(self._h), "ocean_generator_build_mips")

    def mip_levels(self) -> int:
        return int(lib().ocean_generator_mip_levels(self._h))

    def _mip_host(self, getter: str, cascade: int, level: int, channels: int) -> np.ndarray:
        ptr = getattr(lib(), getter)(self._h, int(cascade), int(level))
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, getter)
        self.fft.synchronize()
        side = self.n >> level
        return hip.to_host(int(ptr), (side, side, channels) if channels > 1 else (side, side))

    def height_mip_host(self, cascade: int, level: int) -> np.ndarray:
        return self._mip_host("ocean_generator_height_mip", cascade, level, 4)

    def displacement_mip_host(self, cascade: int, level: int) -> np.ndarray:
        return self._mip_host("ocean_generator_displacement_mip", cascade, level, 4)

    def jacobian_mip_host(self, cascade: int, level: int) -> np.ndarray:
        return self._mip_host("ocean_generator_jacobian_mip", cascade, level, 1)

    # ---- time derivative of the maps (ocean_generator_calculate_rates, include/oceanfft.h) ----
    def calculate_rates(self) -> None:
        """Enqueue d/dt of every cascade's heightMap and displacementMap at the time of the last frame."""
        check(lib().ocean_generator_calculate_rates(self._h), "ocean_generator_calculate_rates")

    def _rate_host(self, getter: str, cascade: int) -> np.ndarray:
        ptr = getattr(lib(), getter)(self._h, int(cascade))
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, getter)
        self.fft.synchronize()
        return hip.to_host(int(ptr), (self.n, self.n, 4))

    def height_rate_map_host(self, cascade: int = 0) -> np.ndarray:
        """d/dt (h, dh/dx, dh/dz, Dx)"""
        return self._rate_host("ocean_generator_height_rate_map", cascade)

    def displacement_rate_map_host(self, cascade: int = 0) -> np.ndarray:
        """d/dt (Dz, dDx/dx, dDz/dz, dDx/dz)"""
        return self._rate_host("ocean_generator_displacement_rate_map", cascade)

    # ---- depth layers (ocean_generator_set_depth_layers / _calculate_kinematics, include/oceanfft.h) ----
    def set_depth_layers(self, depths) -> None:
        """The rest depths in metres below the mean water level: 1..8, finite, >= 0, strictly ascending."""
        d = np.ascontiguousarray(depths, np.float32).reshape(-1)
        check(lib().ocean_generator_set_depth_layers(self._h, d.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     int(d.shape[0])), "ocean_generator_set_depth_layers")

    def depth_layers(self) -> np.ndarray:
        out = np.zeros(8, np.float32)
        count = int(lib().ocean_generator_depth_layers(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out[:count]

    def calculate_kinematics(self) -> None:
        """Enqueue the water velocity and pressure head of every cascade at every depth layer, at the time of
        the last frame."""
        check(lib().ocean_generator_calculate_kinematics(self._h), "ocean_generator_calculate_kinematics")

    def GetKinematicsMap(self, cascade: int = 0, layer: int = 0, image: int = 0) -> int:
        ptr = lib().ocean_generator_kinematics_map(self._h, int(cascade), int(layer), int(image))
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_kinematics_map")
        return int(ptr)

    def kinematics_map_host(self, cascade: int = 0, layer: int = 0, image: int = 0) -> np.ndarray:
        """image 0: (vertical velocity, its x-slope, partner, d/dt Dx); image 1: (d/dt Dz, partner, pressure
        head, its x-slope), at depth layer `layer`."""
        ptr = self.GetKinematicsMap(cascade, layer, image)
        self.fft.synchronize()
        return hip.to_host(ptr, (self.n, self.n, 4))

    # ---- bounds of the maps (ocean_generator_build_bounds, include/oceanfft.h) ----
    def BuildBounds(self) -> None:
        """Enqueue the (min, max) of the nine map channels of every cascade from the current maps."""
        check(lib().ocean_generator_build_bounds(self._h), "ocean_generator_build_bounds")

    build_bounds = BuildBounds

    def GetBounds(self, cascade: int = 0) -> np.ndarray:
        """(9, 2) float32: (min, max) of heightMap x, y, z, w, displacementMap x, y, z, w and the Jacobian."""
        out = np.zeros(18, np.float32)
        check(lib().ocean_generator_bounds(self._h, int(cascade), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
              "ocean_generator_bounds")
        return out.reshape(9, 2)

    get_bounds = GetBounds

    def bounds_device(self) -> int:
        """The table [cascade][18] in device memory (built and fresh, else OceanError)."""
        ptr = lib().ocean_generator_bounds_device(self._h)
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_bounds_device")
        return int(ptr)

    # ---- persistent foam (ocean_generator_advance_foam, include/oceanfft.h) ----
    def AdvanceFoam(self, dt: float) -> None:
        """Enqueue one step of every cascade's foam map from the current Jacobian maps; call it after
        CalculateOcean(dt)."""
        check(lib().ocean_generator_advance_foam(self._h, ctypes.c_float(dt)), "ocean_generator_advance_foam")

    advance_foam = AdvanceFoam

    def ResetFoam(self) -> None:
        """Enqueue the zeroing of the foam maps and the counts."""
        check(lib().ocean_generator_reset_foam(self._h), "ocean_generator_reset_foam")

    reset_foam = ResetFoam

    def GetFoamSettings(self, cascade: int = 0) -> OceanFoamSettings:
        p = lib().ocean_generator_foam_settings(self._h, cascade)
        if not p:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_foam_settings")
        return p.contents

    get_foam_settings = GetFoamSettings

    def GetFoamMap(self, cascade: int = 0) -> int:
        """The R32F N x N foam map in device memory (OceanError before the first AdvanceFoam / ResetFoam)."""
        ptr = lib().ocean_generator_foam_map(self._h, int(cascade))
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_foam_map")
        return int(ptr)

    def foam_map_host(self, cascade: int = 0) -> np.ndarray:
        ptr = self.GetFoamMap(cascade)
        self.fft.synchronize()
        return hip.to_host(ptr, (self.n, self.n))

    def GetFoamCounts(self, cascade: int = 0) -> np.ndarray:
        """(3,) int64: texels of the last step that were breaking (J < bias), covered (foam >= level) and
        saturated (clamped at 1)."""
        out = np.zeros(3, np.int64)
        check(lib().ocean_generator_foam_counts(self._h, int(cascade), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
              "ocean_generator_foam_counts")
        return out

    get_foam_counts = GetFoamCounts

    def foam_counts_device(self) -> int:
        """The int64 table [cascade][3] in device memory (OceanError before the first AdvanceFoam / ResetFoam)."""
        ptr = lib().ocean_generator_foam_counts_device(self._h)
        if not ptr:
            raise capi.OceanError(capi.OCEAN_ERR_INVALID, "ocean_generator_foam_counts_device")
        return int(ptr)

    # ---- instrumentation ----
    def set_profiling(self, enable: bool) -> None:
        check(lib().ocean_generator_set_profiling(self._h, 1 if enable else 0), "ocean_generator_set_profiling")

    def kernel_times(self):
        """(ms totals, launch counts) for [spectrum, column pass, row pass] since the last call."""
        ms = (ctypes.c_double * 3)()
        cnt = (ctypes.c_int64 * 3)()
        check(lib().ocean_generator_kernel_times(self._h, ms, cnt), "ocean_generator_kernel_times")
        return list(ms), list(cnt)

    def close(self) -> None:
        if self._h:
            lib().ocean_generator_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_copy(dst_ptr: int, src_ptr: int, nbytes: int, workgroups: int, stream: int | None = None) -> None:
    """ocean_debug_copy: a copy on exactly `workgroups` 256-thread workgroups (a rate-limited HBM stream)."""
    check(lib().ocean_debug_copy(ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), nbytes, workgroups,
                                 ctypes.c_void_p(stream or 0)), "ocean_debug_copy")


def debug_hash(xy_dev_ptr: int, count: int, raw_dev_ptr: int, uv_dev_ptr: int, stream: int | None = None) -> None:
    check(lib().ocean_debug_hash(ctypes.c_void_p(xy_dev_ptr), count, ctypes.c_void_p(raw_dev_ptr),
                                 ctypes.c_void_p(uv_dev_ptr), ctypes.c_void_p(stream or 0)), "ocean_debug_hash")
