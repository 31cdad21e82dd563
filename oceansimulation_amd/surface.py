"""Surface consumer of the generator maps: resources/waveShader.glsl's vertex
displacement (:101-110) and fragment slope normal / Jacobian (:127-144), per mesh vertex, through
ocean_surface_sample / ocean_surface_sample_plane, and the opposite direction, the water surface above
world positions, through ocean_surface_query, the water below the surface at world positions through
ocean_water_kinematics, and the loads on floating bodies built on both, ocean_hulls_loads
(include/oceanfft.h)."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import hip
from .capi import (OCEAN_ERR_INVALID, OceanCamera, OceanCameraLayers, OceanError, OceanFoamDepositSettings, OceanMarch,
                   OceanHullStepSettings, OceanMooringSettings, OceanShading, OceanSpraySettings, check, lib)
from .hip import DeviceBuffer

FLOATS_PER_VERTEX = 8  # x, y, z, jacobian, nx, ny, nz, 0 (query: base x, height, base z, ..., residual)
FLOATS_PER_RAY = 8     # ox, oy, oz, tmin, dx, dy, dz, tmax
FLOATS_PER_HIT = 16    # ocean_surface_raycast's four rows
FLOATS_PER_WATER_POINT = 12  # ocean_water_kinematics' three rows
RAY_HIT, RAY_OUTSIDE, RAY_EXIT, RAY_STEP_LIMIT = 0, 1, 2, 3
DEPOSIT_COUNTS = 50  # ocean_foam_deposit: n, offered, then (taps, touched, saturated) per pair
DEPOSIT_ITEM = 256   # records per work item of the deposit's kernels (kFoamDepositItem)


def default_camera() -> OceanCamera:
    c = OceanCamera()
    lib().ocean_default_camera(ctypes.byref(c))
    return c


def default_shading(**overrides) -> OceanShading:
    s = OceanShading()
    lib().ocean_default_shading(ctypes.byref(s))
    _set_fields(s, overrides)
    return s


def default_march(**overrides) -> OceanMarch:
    m = OceanMarch()
    lib().ocean_default_march(ctypes.byref(m))
    _set_fields(m, overrides)
    return m


def default_camera_layers(**overrides) -> OceanCameraLayers:
    l = OceanCameraLayers()
    lib().ocean_default_camera_layers(ctypes.byref(l))
    _set_fields(l, overrides)
    return l


def _set_fields(struct, values) -> None:
    names = {f[0] for f in struct._fields_}
    for k, v in values.items():
        if k not in names:
            raise AttributeError(f"{type(struct).__name__} has no field {k!r}")
        if isinstance(getattr(struct, k), ctypes.Array):
            v = type(getattr(struct, k))(*[float(x) for x in v])
        setattr(struct, k, v)


def camera_pose(position, pitch_deg: float, yaw_deg: float, fov_y_deg: float, near: float, far: float,
                lod_scale: float = 0.0) -> OceanCamera:
    """An ocean_camera from the reference's camera angles (src/Renderer.cpp:15-16), with ocean_default_camera's
    convention evaluated in double and rounded once: forward = (cos p sin y, sin p, -cos p cos y),
    right = (cos y, 0, sin y), up = right x forward."""
    p, y = math.radians(pitch_deg), math.radians(yaw_deg)
    f = (math.cos(p) * math.sin(y), math.sin(p), -math.cos(p) * math.cos(y))
    r = (math.cos(y), 0.0, math.sin(y))
    u = (r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0])
    c = OceanCamera()
    _set_fields(c, dict(position=position, right=r, up=u, forward=f,
                        tan_half_fov_y=math.tan(math.radians(fov_y_deg) / 2.0), near_plane=near, far_plane=far,
                        lod_scale=lod_scale))
    return c


def camera_layers_scratch_bytes(width: int, height: int) -> int:
    """Bytes of ocean_camera_render_layers' scratch for a width x height image."""
    return int(lib().ocean_camera_layers_scratch_bytes(int(width), int(height)))


def camera_rays_host(camera: OceanCamera, width: int, height: int) -> np.ndarray:
    """ocean_camera_rays on the default stream -> (height * width, 8) float32, row 0 the top row."""
    n = int(width) * int(height)
    out = DeviceBuffer(max(n, 1) * FLOATS_PER_RAY * 4)
    check(lib().ocean_camera_rays(ctypes.byref(camera), int(width), int(height), ctypes.c_void_p(out.ptr), None),
          "ocean_camera_rays")
    hip.synchronize()
    return out.to_host((n, FLOATS_PER_RAY))


class SurfaceSampler:
    """The renderer's view of `pairs` = [(Generator, cascade), ...] (src/Renderer.cpp:62-72)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)
        n = len(self.pairs)
        self._gens = (ctypes.c_void_p * n)(*[g.handle.value for g, _ in self.pairs])
        self._cas = (ctypes.c_int * n)(*[int(c) for _, c in self.pairs])
        self.fft = self.pairs[0][0].fft

    def sample(self, xz_ptr: int, points: int, out_ptr: int) -> None:
        check(lib().ocean_surface_sample(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xz_ptr),
                                         ctypes.c_int64(points), ctypes.c_void_p(out_ptr)), "ocean_surface_sample")

    def sample_plane(self, camera, res: int, out_ptr: int) -> None:
        cam = (ctypes.c_float * 5)(*[float(v) for v in camera])
        check(lib().ocean_surface_sample_plane(self._gens, self._cas, len(self.pairs), cam, int(res),
                                               ctypes.c_void_p(out_ptr)), "ocean_surface_sample_plane")

    def query(self, xz_ptr: int, points: int, iterations: int, tolerance: float, out_ptr: int) -> None:
        check(lib().ocean_surface_query(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xz_ptr),
                                        ctypes.c_int64(points), int(iterations), ctypes.c_float(tolerance),
                                        ctypes.c_void_p(out_ptr)), "ocean_surface_query")

    def sample_host(self, xz: np.ndarray) -> np.ndarray:
        xz = np.ascontiguousarray(xz, np.float32)
        pts = xz.shape[0]
        src = DeviceBuffer.from_array(xz)
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4)
        self.sample(src.ptr, pts, out.ptr)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX))

    def query_host(self, xz: np.ndarray, iterations: int = 8, tolerance: float = 0.0) -> np.ndarray:
        """Per world position (x, z): (base x, water height, base z, jacobian, nx, ny, nz, residual in m)."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        pts = xz.shape[0]
        src = DeviceBuffer.from_array(xz) if pts else None
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4) if pts else None
        self.query(src.ptr if pts else 0, pts, iterations, tolerance, out.ptr if pts else 0)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX)) if pts else np.zeros((0, FLOATS_PER_VERTEX), np.float32)

    # ---- persistent foam in slot 7 (Generator.AdvanceFoam or ResetFoam first) ----
    def sample_foam_device(self, xz_ptr: int, points: int, out_ptr: int) -> None:
        check(lib().ocean_surface_sample_foam(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xz_ptr),
                                              ctypes.c_int64(points), ctypes.c_void_p(out_ptr)),
              "ocean_surface_sample_foam")

    def sample_plane_foam_device(self, camera, res: int, out_ptr: int) -> None:
        cam = (ctypes.c_float * 5)(*[float(v) for v in camera])
        check(lib().ocean_surface_sample_plane_foam(self._gens, self._cas, len(self.pairs), cam, int(res),
                                                    ctypes.c_void_p(out_ptr)), "ocean_surface_sample_plane_foam")

    def sample_foam(self, xz: np.ndarray) -> np.ndarray:
        """Per base point (x, z): ocean_surface_sample's 8 floats with the cascades' averaged foam in slot 7."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        pts = xz.shape[0]
        src = DeviceBuffer.from_array(xz) if pts else None
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4) if pts else None
        self.sample_foam_device(src.ptr if pts else 0, pts, out.ptr if pts else 0)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX)) if pts else np.zeros((0, FLOATS_PER_VERTEX), np.float32)

    def sample_plane_foam(self, camera, res: int) -> np.ndarray:
        """The plane mesh through the camera warp, foam in slot 7 -> ((res + 1)^2, 8)."""
        pts = (res + 1) * (res + 1)
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4)
        self.sample_plane_foam_device(camera, res, out.ptr)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX))

    # ---- spray impacts into the persistent foam (Generator.AdvanceFoam or ResetFoam first) ----
    def _deposit_settings(self, settings):
        n = len(self.pairs)
        if isinstance(settings, (OceanFoamDepositSettings, dict)):
            settings = [settings] * n
        if len(settings) != n:
            raise ValueError("one ocean_foam_deposit_settings per (generator, cascade) pair")
        arr = (OceanFoamDepositSettings * n)()
        for i, s in enumerate(settings):
            if isinstance(s, dict):
                lib().ocean_default_foam_deposit_settings(ctypes.byref(arr[i]))
                for k, v in s.items():
                    if k not in ("amount", "per_speed"):
                        raise AttributeError(f"ocean_foam_deposit_settings has no field {k!r}")
                    setattr(arr[i], k, v)
            else:
                arr[i] = OceanFoamDepositSettings(s.amount, s.per_speed)
        return arr

    def deposit_foam(self, records_ptr: int, max_records: int, settings, count_device: int = 0) -> None:
        """Enqueue ocean_foam_deposit on the plan's stream: device records (max_records, 8) in the layout of a
        particle step's impacts, counted by the int64 at count_device (SprayParticles.counts_device() + 32 for an
        impact list; 0: all max_records). settings: one OceanFoamDepositSettings or dict of its fields for every
        pair, or a list of them."""
        arr = self._deposit_settings(settings)
        check(lib().ocean_foam_deposit(self._gens, self._cas, len(self.pairs), arr, ctypes.c_void_p(records_ptr or 0),
                                       ctypes.c_void_p(count_device or 0), ctypes.c_int64(max_records)),
              "ocean_foam_deposit")

    def deposit_foam_host(self, records: np.ndarray, settings) -> np.ndarray:
        """Deposit host records (n, 8) of 4-byte words, all of them; returns deposit_counts()."""
        records = np.ascontiguousarray(records).reshape(-1, FLOATS_PER_VERTEX)
        assert records.dtype.itemsize == 4
        src = DeviceBuffer.from_array(records) if records.shape[0] else None
        self.deposit_foam(src.ptr if src else 0, records.shape[0], settings)
        return self.deposit_counts()  # synchronises: src is freed on return

    def deposit_counts(self) -> np.ndarray:
        """The int64[50] counts of the last deposit on the host (n, offered, then taps, touched, saturated per
        pair); synchronises the plan's stream."""
        out = (ctypes.c_int64 * DEPOSIT_COUNTS)()
        check(lib().ocean_foam_deposit_counts(self._gens[0], out), "ocean_foam_deposit_counts")
        return np.array(out[:], np.int64)

    def deposit_counts_device(self) -> int:
        ptr = lib().ocean_foam_deposit_counts_device(self._gens[0])
        if not ptr:
            raise OceanError(OCEAN_ERR_INVALID, "ocean_foam_deposit_counts_device")
        return int(ptr)

    # ---- footprint-aware sampling of the mip pyramids (Generator.build_mips first) ----
    def sample_lod(self, xzf_ptr: int, points: int, out_ptr: int) -> None:
        check(lib().ocean_surface_sample_lod(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xzf_ptr),
                                             ctypes.c_int64(points), ctypes.c_void_p(out_ptr)),
              "ocean_surface_sample_lod")

    def sample_plane_lod(self, camera, res: int, out_ptr: int) -> None:
        cam = (ctypes.c_float * 5)(*[float(v) for v in camera])
        check(lib().ocean_surface_sample_plane_lod(self._gens, self._cas, len(self.pairs), cam, int(res),
                                                   ctypes.c_void_p(out_ptr)), "ocean_surface_sample_plane_lod")

    def sample_lod_host(self, xzf: np.ndarray) -> np.ndarray:
        """Per (x, z, footprint in m): ocean_surface_sample's 8 floats, slot 7 = the footprint."""
        xzf = np.ascontiguousarray(xzf, np.float32).reshape(-1, 3)
        pts = xzf.shape[0]
        src = DeviceBuffer.from_array(xzf) if pts else None
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4) if pts else None
        self.sample_lod(src.ptr if pts else 0, pts, out.ptr if pts else 0)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX)) if pts else np.zeros((0, FLOATS_PER_VERTEX), np.float32)

    def plane_lod_host(self, camera, res: int) -> np.ndarray:
        pts = (res + 1) * (res + 1)
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4)
        self.sample_plane_lod(camera, res, out.ptr)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX))

    # ---- velocity of water particles (Generator.calculate_rates first) ----
    def velocity(self, xz_ptr: int, points: int, out_ptr: int) -> None:
        check(lib().ocean_surface_velocity(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xz_ptr),
                                           ctypes.c_int64(points), ctypes.c_void_p(out_ptr)), "ocean_surface_velocity")

    def velocity_host(self, xz: np.ndarray) -> np.ndarray:
        """Per base point (x, z): (displaced x, y, z, 0, velocity x, y, z in m/s, 0)."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        pts = xz.shape[0]
        src = DeviceBuffer.from_array(xz) if pts else None
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4) if pts else None
        self.velocity(src.ptr if pts else 0, pts, out.ptr if pts else 0)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX)) if pts else np.zeros((0, FLOATS_PER_VERTEX), np.float32)

    # ---- the water below the surface (Generator.set_depth_layers and calculate_kinematics first) ----
    def kinematics(self, xyz_ptr: int, points: int, iterations: int, tolerance: float, out_ptr: int) -> None:
        """Enqueue ocean_water_kinematics: device positions (n, 3) -> device rows (n, 12)."""
        check(lib().ocean_water_kinematics(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(xyz_ptr),
                                           ctypes.c_int64(points), int(iterations), ctypes.c_float(tolerance),
                                           ctypes.c_void_p(out_ptr)), "ocean_water_kinematics")

    def kinematics_host(self, xyz: np.ndarray, iterations: int = 8, tolerance: float = 0.0) -> np.ndarray:
        """Per world position (x, y, z): (base x, water height, base z, residual, velocity x, y, z in m/s,
        pressure head in m, depth under the surface, layer, blend factor, wet)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        pts = xyz.shape[0]
        src = DeviceBuffer.from_array(xyz) if pts else None
        out = DeviceBuffer(pts * FLOATS_PER_WATER_POINT * 4) if pts else None
        self.kinematics(src.ptr if pts else 0, pts, iterations, tolerance, out.ptr if pts else 0)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_WATER_POINT)) if pts else np.zeros((0, FLOATS_PER_WATER_POINT), np.float32)

    # ---- ray casting against the displaced surface (Generator.BuildBounds first) ----
    def raycast(self, rays_ptr: int, n_rays: int, out_ptr: int, step: float = 0.25, max_steps: int = 256,
                refine: int = 10, iterations: int = 4, tolerance: float = 1e-3, slope: float = float("inf"),
                pad: float = 0.0) -> None:
        """Enqueue ocean_surface_raycast: device rays (n, 8) -> device rows (n, 16)."""
        check(lib().ocean_surface_raycast(self._gens, self._cas, len(self.pairs), ctypes.c_void_p(rays_ptr),
                                          ctypes.c_int64(n_rays), ctypes.c_float(step), int(max_steps), int(refine),
                                          int(iterations), ctypes.c_float(tolerance), ctypes.c_float(slope),
                                          ctypes.c_float(pad), ctypes.c_void_p(out_ptr)), "ocean_surface_raycast")

    def raycast_host(self, rays: np.ndarray, step: float = 0.25, max_steps: int = 256, refine: int = 10,
                     iterations: int = 4, tolerance: float = 1e-3, slope: float = float("inf"),
                     pad: float = 0.0) -> np.ndarray:
        """Per ray (ox, oy, oz, tmin, dx, dy, dz, tmax): 16 floats, (hit point, t), (normal, jacobian),
        (base x, water height, base z, residual), (status, below, steps, gap); include/oceanfft.h."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, FLOATS_PER_RAY)
        n = rays.shape[0]
        src = DeviceBuffer.from_array(rays) if n else None
        out = DeviceBuffer(n * FLOATS_PER_HIT * 4) if n else None
        self.raycast(src.ptr if n else 0, n, out.ptr if n else 0, step, max_steps, refine, iterations, tolerance,
                     slope, pad)
        self.fft.synchronize()
        return out.to_host((n, FLOATS_PER_HIT)) if n else np.zeros((0, FLOATS_PER_HIT), np.float32)

    # ---- camera images (Generator.BuildBounds first; with camera.lod_scale > 0 also Generator.build_mips) ----
    def render(self, camera: OceanCamera, shading: OceanShading, march: OceanMarch, width: int, height: int,
               image_ptr: int = 0, aux_ptr: int = 0, image8_ptr: int = 0) -> None:
        """Enqueue ocean_camera_render: device image (h, w, 4) float32, aux (h, w, 4) float32 (t, depth, jacobian,
        status) and image8 (h, w, 4) uint8, any of them 0 (not all)."""
        check(lib().ocean_camera_render(self._gens, self._cas, len(self.pairs), ctypes.byref(camera),
                                        ctypes.byref(shading), ctypes.byref(march), int(width), int(height),
                                        ctypes.c_void_p(image_ptr), ctypes.c_void_p(aux_ptr),
                                        ctypes.c_void_p(image8_ptr)), "ocean_camera_render")

    def render_host(self, camera: OceanCamera, width: int, height: int, shading: OceanShading = None,
                    march: OceanMarch = None):
        """(image (h, w, 4) float32, aux (h, w, 4) float32, image8 (h, w, 4) uint8) of one camera."""
        shading = default_shading() if shading is None else shading
        march = default_march() if march is None else march
        n = int(width) * int(height)
        image, aux, image8 = DeviceBuffer(max(n, 1) * 16), DeviceBuffer(max(n, 1) * 16), DeviceBuffer(max(n, 1) * 4)
        self.render(camera, shading, march, width, height, image.ptr, aux.ptr, image8.ptr)
        self.fft.synchronize()
        return (image.to_host((height, width, 4)), aux.to_host((height, width, 4)),
                image8.to_host((height, width, 4), np.uint8))

    # ---- camera images with foam and spray (with layers.foam_opacity > 0: Generator.AdvanceFoam or ResetFoam) ----
    def render_layers(self, camera: OceanCamera, shading: OceanShading, march: OceanMarch, layers: OceanCameraLayers,
                      width: int, height: int, image_ptr: int = 0, aux_ptr: int = 0, aux2_ptr: int = 0,
                      image8_ptr: int = 0, particles: "SprayParticles" = None, records_ptr: int = 0,
                      count_ptr: int = 0, max_records: int = 0, scratch_ptr: int = 0) -> None:
        """Enqueue ocean_camera_render_layers: render's outputs and aux2 (h, w, 4) float32 (foam, spray depth,
        hit count and nearest record index as uint32 bits), any of them 0 (not all). The spray is a
        SprayParticles pool (its list, counted by its device table), or device records (max_records, 8) with a
        device int64 count (0: all of them); either needs scratch_ptr, camera_layers_scratch_bytes(w, h) bytes."""
        if particles is not None:
            records_ptr, count_ptr, max_records = particles.records_ptr, particles.counts_device(), particles.capacity
        check(lib().ocean_camera_render_layers(self._gens, self._cas, len(self.pairs), ctypes.byref(camera),
                                               ctypes.byref(shading), ctypes.byref(march), ctypes.byref(layers),
                                               int(width), int(height), ctypes.c_void_p(records_ptr),
                                               ctypes.c_void_p(count_ptr), ctypes.c_int64(max_records),
                                               ctypes.c_void_p(scratch_ptr), ctypes.c_void_p(image_ptr),
                                               ctypes.c_void_p(aux_ptr), ctypes.c_void_p(aux2_ptr),
                                               ctypes.c_void_p(image8_ptr)), "ocean_camera_render_layers")

    def render_layers_host(self, camera: OceanCamera, width: int, height: int, layers: OceanCameraLayers = None,
                           shading: OceanShading = None, march: OceanMarch = None,
                           particles: "SprayParticles" = None, records: np.ndarray = None, count: int = None):
        """(image, aux, aux2 (h, w, 4) float32, image8 (h, w, 4) uint8) of one camera. The spray: a SprayParticles
        pool, or host records (n, 8) of which the first `count` are used (a device count; None: all n)."""
        layers = default_camera_layers() if layers is None else layers
        shading = default_shading() if shading is None else shading
        march = default_march() if march is None else march
        n = int(width) * int(height)
        image, aux, aux2 = (DeviceBuffer(max(n, 1) * 16) for _ in range(3))
        image8 = DeviceBuffer(max(n, 1) * 4)
        rec = cnt = scratch = None
        max_records = 0
        if records is not None:
            records = np.ascontiguousarray(records).reshape(-1, FLOATS_PER_VERTEX)
            assert records.dtype.itemsize == 4
            max_records = records.shape[0]
            rec = DeviceBuffer.from_array(records) if max_records else None
            if count is not None:
                cnt = DeviceBuffer.from_array(np.array([count], np.int64))
        if particles is not None or max_records:
            scratch = DeviceBuffer(camera_layers_scratch_bytes(width, height))
        self.render_layers(camera, shading, march, layers, width, height, image.ptr, aux.ptr, aux2.ptr, image8.ptr,
                           particles=particles, records_ptr=rec.ptr if rec else 0, count_ptr=cnt.ptr if cnt else 0,
                           max_records=max_records, scratch_ptr=scratch.ptr if scratch else 0)
        self.fft.synchronize()
        return (image.to_host((height, width, 4)), aux.to_host((height, width, 4)), aux2.to_host((height, width, 4)),
                image8.to_host((height, width, 4), np.uint8))

    def plane_host(self, camera, res: int) -> np.ndarray:
        pts = (res + 1) * (res + 1)
        out = DeviceBuffer(pts * FLOATS_PER_VERTEX * 4)
        self.sample_plane(camera, res, out.ptr)
        self.fft.synchronize()
        return out.to_host((pts, FLOATS_PER_VERTEX))


class HullSet:
    """Floating bodies as sets of hull points (ocean_hulls, include/oceanfft.h). points: (P, 8) float32
    (lx, ly, lz, volume, half_height, drag_lin, drag_quad, 0) in the body frame; ranges: (bodies, 2) int32
    (first, count) into points, which bodies may share."""

    def __init__(self, fft, points: np.ndarray, ranges: np.ndarray):
        self._points = np.ascontiguousarray(points, np.float32).reshape(-1, FLOATS_PER_VERTEX)
        self._ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 2)
        self.fft = fft
        h = ctypes.c_void_p()
        check(lib().ocean_hulls_create(ctypes.byref(h), fft.handle, self._points.ctypes.data,
                                       ctypes.c_int64(self._points.shape[0]), self._ranges.ctypes.data,
                                       self._ranges.shape[0]), "ocean_hulls_create")
        self._h = h
        self.bodies = int(lib().ocean_hulls_bodies(h))
        self.instance_points = int(lib().ocean_hulls_instance_points(h))

    @property
    def handle(self):
        return self._h

    def loads(self, sampler: SurfaceSampler, poses_ptr: int, loads_ptr: int, point_out_ptr: int = 0,
              rho_g: float = 9810.0, iterations: int = 8, tolerance: float = 0.0, water_velocity: bool = False) -> None:
        """Enqueue one step on the plan's stream: device poses (bodies, 20) -> device loads (bodies, 8) and,
        with point_out_ptr, the per-point rows (instance_points, 8)."""
        check(lib().ocean_hulls_loads(self._h, sampler._gens, sampler._cas, len(sampler.pairs),
                                      ctypes.c_void_p(poses_ptr), ctypes.c_float(rho_g), int(iterations),
                                      ctypes.c_float(tolerance), int(water_velocity), ctypes.c_void_p(loads_ptr),
                                      ctypes.c_void_p(point_out_ptr)), "ocean_hulls_loads")

    def loads_host(self, sampler: SurfaceSampler, poses: np.ndarray, rho_g: float = 9810.0, iterations: int = 8,
                   tolerance: float = 0.0, water_velocity: bool = False):
        """(loads (bodies, 8), point_out (instance_points, 8)) of host poses (bodies, 20)."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(self.bodies, 20)
        src = DeviceBuffer.from_array(poses)
        out = DeviceBuffer(self.bodies * FLOATS_PER_VERTEX * 4)
        pts = DeviceBuffer(self.instance_points * FLOATS_PER_VERTEX * 4)
        self.loads(sampler, src.ptr, out.ptr, pts.ptr, rho_g, iterations, tolerance, water_velocity)
        self.fft.synchronize()
        return out.to_host((self.bodies, FLOATS_PER_VERTEX)), pts.to_host((self.instance_points, FLOATS_PER_VERTEX))

    def set_bodies(self, props: np.ndarray) -> None:
        """props: (bodies, 8) float32 (mass, Ix, Iy, Iz, lin_damp, ang_damp, kinematic, 0); what step needs."""
        props = np.ascontiguousarray(props, np.float32).reshape(self.bodies, FLOATS_PER_VERTEX)
        check(lib().ocean_hulls_set_bodies(self._h, props.ctypes.data), "ocean_hulls_set_bodies")

    @staticmethod
    def step_settings(**overrides) -> OceanHullStepSettings:
        """The library's defaults with `overrides` (dt, substeps, gravity, rho_g, iterations, tolerance,
        water_velocity)."""
        s = OceanHullStepSettings()
        lib().ocean_default_hull_step_settings(ctypes.byref(s))
        for k, v in overrides.items():
            if k == "gravity":
                s.gravity[:] = [float(x) for x in v]
            elif k in ("substeps", "iterations", "water_velocity"):
                setattr(s, k, int(v))
            else:
                getattr(OceanHullStepSettings, k)  # an unknown name is an AttributeError
                setattr(s, k, float(v))
        return s

    def step(self, sampler: SurfaceSampler, poses_ptr: int, settings: OceanHullStepSettings = None, ext_ptr: int = 0,
             loads_ptr: int = 0, point_out_ptr: int = 0, **overrides) -> None:
        """Enqueue one ocean_hulls_step on the plan's stream: the device poses (bodies, 20) are stepped in place
        by settings.dt in settings.substeps substeps under the wave loads, gravity and the device wrenches at
        ext_ptr (bodies, 8); loads_ptr and point_out_ptr receive the last substep's loads. `overrides` are
        fields of the settings (step_settings)."""
        if settings is None:
            settings = self.step_settings(**overrides)
        elif overrides:
            raise TypeError("HullSet.step: pass settings or their fields, not both")
        check(lib().ocean_hulls_step(self._h, sampler._gens, sampler._cas, len(sampler.pairs), ctypes.byref(settings),
                                     ctypes.c_void_p(poses_ptr), ctypes.c_void_p(ext_ptr), ctypes.c_void_p(loads_ptr),
                                     ctypes.c_void_p(point_out_ptr)), "ocean_hulls_step")

    def step_host(self, sampler: SurfaceSampler, poses: np.ndarray, settings: OceanHullStepSettings = None,
                  ext: np.ndarray = None, calls: int = 1, **overrides):
        """`calls` successive steps of host poses (bodies, 20): a list of (poses, loads, point_out) after each."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(self.bodies, 20)
        buf = DeviceBuffer.from_array(poses)
        e = DeviceBuffer.from_array(np.ascontiguousarray(ext, np.float32).reshape(self.bodies, 8)) if ext is not None else None
        out = DeviceBuffer(self.bodies * FLOATS_PER_VERTEX * 4)
        pts = DeviceBuffer(self.instance_points * FLOATS_PER_VERTEX * 4)
        results = []
        for _ in range(calls):
            self.step(sampler, buf.ptr, settings, e.ptr if e else 0, out.ptr, pts.ptr, **overrides)
            self.fft.synchronize()
            results.append((buf.to_host((self.bodies, 20)), out.to_host((self.bodies, FLOATS_PER_VERTEX)),
                            pts.to_host((self.instance_points, FLOATS_PER_VERTEX))))
        return results

    def close(self) -> None:
        if self._h:
            lib().ocean_hulls_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MooringSet:
    """Mooring lines (ocean_moorings, include/oceanfft.h): chains of lumped nodes between anchors fixed in the
    world and fairleads on the bodies of a hull set. lines: (L, 16) float32 (anchor, fairlead, length, EA, CA,
    mass_per_m, volume_per_m, drag_lin, drag_quad, 0, 0, 0); attach: (L, 2) int32 (body or -1, nodes 2..64)."""

    def __init__(self, fft, lines: np.ndarray, attach: np.ndarray, bodies: int):
        self._lines = np.ascontiguousarray(lines, np.float32).reshape(-1, 16)
        self._attach = np.ascontiguousarray(attach, np.int32).reshape(-1, 2)
        self.fft = fft
        self.bodies = int(bodies)
        h = ctypes.c_void_p()
        check(lib().ocean_moorings_create(ctypes.byref(h), fft.handle, self._lines.ctypes.data, self._attach.ctypes.data,
                                          self._lines.shape[0], self.bodies), "ocean_moorings_create")
        self._h = h
        self.lines = int(lib().ocean_moorings_lines(h))
        self.total_nodes = int(lib().ocean_moorings_total_nodes(h))

    @property
    def handle(self):
        return self._h

    @property
    def nodes_ptr(self) -> int:
        """The device nodes (total_nodes, 8), for the caller to read and write on the plan's stream."""
        return int(lib().ocean_moorings_nodes(self._h) or 0)

    @staticmethod
    def settings(**overrides) -> OceanMooringSettings:
        """The library's defaults with `overrides` (dt, substeps, gravity, rho_g, iterations, tolerance, water,
        bed_y, bed_k, bed_c)."""
        s = OceanMooringSettings()
        lib().ocean_default_mooring_settings(ctypes.byref(s))
        for k, v in overrides.items():
            if k == "gravity":
                s.gravity[:] = [float(x) for x in v]
            elif k in ("substeps", "iterations", "water"):
                setattr(s, k, int(v))
            else:
                getattr(OceanMooringSettings, k)  # an unknown name is an AttributeError
                setattr(s, k, float(v))
        return s

    def reset(self, poses_ptr: int = 0) -> None:
        """Enqueue ocean_moorings_reset: every line straight from its anchor to its fairlead, at rest."""
        check(lib().ocean_moorings_reset(self._h, ctypes.c_void_p(poses_ptr)), "ocean_moorings_reset")

    def step(self, sampler: "SurfaceSampler" = None, poses_ptr: int = 0, wrench_ptr: int = 0, line_out_ptr: int = 0,
             settings: OceanMooringSettings = None, **overrides) -> None:
        """Enqueue one ocean_moorings_step on the plan's stream: the nodes are stepped in place under the frozen
        device poses (bodies, 20); wrench_ptr (bodies, 8) receives ocean_hulls_step's wrench_ext, line_out_ptr
        (lines, 8) the per-line rows. sampler: the water of settings.water == 1 (None for still water).
        `overrides` are fields of the settings."""
        if settings is None:
            settings = self.settings(**overrides)
        elif overrides:
            raise TypeError("MooringSet.step: pass settings or their fields, not both")
        gens, cas, count = (sampler._gens, sampler._cas, len(sampler.pairs)) if sampler is not None else (None, None, 0)
        check(lib().ocean_moorings_step(self._h, gens, cas, count, ctypes.byref(settings), ctypes.c_void_p(poses_ptr),
                                        ctypes.c_void_p(wrench_ptr), ctypes.c_void_p(line_out_ptr)),
              "ocean_moorings_step")

    def nodes_host(self) -> np.ndarray:
        """The nodes (total_nodes, 8) after the stream's work."""
        self.fft.synchronize()
        return hip.to_host(self.nodes_ptr, (self.total_nodes, 8))

    def set_nodes_host(self, nodes: np.ndarray) -> None:
        """Write the nodes (total_nodes, 8) from the host, after the stream's work."""
        nodes = np.ascontiguousarray(nodes, np.float32).reshape(self.total_nodes, 8)
        self.fft.synchronize()
        hip.from_host(self.nodes_ptr, nodes)

    def step_host(self, sampler: "SurfaceSampler" = None, poses: np.ndarray = None, settings: OceanMooringSettings = None,
                  calls: int = 1, **overrides):
        """`calls` successive steps under host poses (bodies, 20): a list of (nodes, line_out, wrench_ext) after
        each; line_out and wrench_ext start as NaN."""
        p = DeviceBuffer.from_array(np.ascontiguousarray(poses, np.float32).reshape(self.bodies, 20)) if self.bodies else None
        nan = np.float32(np.nan)
        results = []
        for _ in range(calls):
            lines = DeviceBuffer.from_array(np.full((self.lines, 8), nan, np.float32))
            wrench = DeviceBuffer.from_array(np.full((self.bodies, 8), nan, np.float32)) if self.bodies else None
            self.step(sampler, p.ptr if p else 0, wrench.ptr if wrench else 0, lines.ptr, settings, **overrides)
            results.append((self.nodes_host(), lines.to_host((self.lines, 8)),
                            wrench.to_host((self.bodies, 8)) if wrench else np.zeros((0, 8), np.float32)))
        return results

    def close(self) -> None:
        if self._h:
            lib().ocean_moorings_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SPRAY_COUNTS = 18  # written, found, found per pair


class SprayEmitter:
    """Emitters at breaking crests (ocean_spray, include/oceanfft.h): the texels of a sampler's pairs whose
    Jacobian is under the pair's threshold, thinned by rate * dt, as an ordered list of 8-float records
    (displaced x, y, z, threshold - J, velocity x, y, z in m/s, id = pair << 28 | texel as uint32 bits)."""

    def __init__(self, fft):
        self.fft = fft
        h = ctypes.c_void_p()
        check(lib().ocean_spray_create(ctypes.byref(h), fft.handle), "ocean_spray_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    @staticmethod
    def _settings(settings, count):
        if isinstance(settings, (OceanSpraySettings, dict)):
            settings = [settings] * count
        arr = (OceanSpraySettings * len(settings))()
        for i, s in enumerate(settings):
            if isinstance(s, dict):
                lib().ocean_default_spray_settings(ctypes.byref(arr[i]))
                for k, v in s.items():
                    if k not in ("threshold", "rate", "seed"):
                        raise AttributeError(f"ocean_spray_settings has no field {k!r}")
                    setattr(arr[i], k, v)
            else:
                arr[i] = OceanSpraySettings(s.threshold, s.rate, s.seed)
        return arr

    def emit(self, sampler: SurfaceSampler, settings, dt: float, step: int, out_ptr: int = 0, capacity: int = 0,
             velocity: bool = True, tiles=None) -> None:
        """Enqueue one call on the plan's stream: device records (capacity, 8), or with capacity 0 the counts
        alone. settings: one OceanSpraySettings or dict of its fields for every pair, or a list of them;
        tiles: (pairs, 2) int32 plane offsets or None."""
        n = len(sampler.pairs)
        arr = self._settings(settings, n)
        if len(arr) != n:
            raise ValueError("one ocean_spray_settings per (generator, cascade) pair")
        t = None
        if tiles is not None:
            t = np.ascontiguousarray(tiles, np.int32).reshape(n, 2)
        check(lib().ocean_spray_emit(self._h, sampler._gens, sampler._cas, n, arr,
                                     ctypes.c_void_p(t.ctypes.data if t is not None else 0), ctypes.c_float(dt),
                                     ctypes.c_uint32(step), int(velocity), ctypes.c_int64(capacity),
                                     ctypes.c_void_p(out_ptr)), "ocean_spray_emit")

    def emit_host(self, sampler: SurfaceSampler, settings, dt: float, step: int, capacity: int, velocity: bool = True,
                  tiles=None):
        """(records (written, 8) float32, counts (18,) int64) of one call with room for `capacity` records."""
        out = DeviceBuffer(capacity * FLOATS_PER_VERTEX * 4) if capacity else None
        self.emit(sampler, settings, dt, step, out.ptr if capacity else 0, capacity, velocity, tiles)
        counts = self.counts()
        if not capacity:
            return np.zeros((0, FLOATS_PER_VERTEX), np.float32), counts
        return out.to_host((capacity, FLOATS_PER_VERTEX))[:int(counts[0])].copy(), counts

    def counts(self) -> np.ndarray:
        """The last call's counts on the host; synchronises the plan's stream."""
        out = (ctypes.c_int64 * SPRAY_COUNTS)()
        check(lib().ocean_spray_counts(self._h, out), "ocean_spray_counts")
        return np.array(out[:], np.int64)

    def counts_device(self) -> int:
        """The int64[18] count table in device memory (OceanError before the first emit)."""
        ptr = lib().ocean_spray_counts_device(self._h)
        if not ptr:
            raise OceanError(OCEAN_ERR_INVALID, "ocean_spray_counts_device")
        return int(ptr)

    def close(self) -> None:
        if self._h:
            lib().ocean_spray_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PARTICLE_COUNTS = 8  # alive, alive before, survivors, landed found, landed written, expired, appended, dropped
PARTICLE_ITEM = 256  # particles per work item of the step's kernels (kParticleItem)


class SprayParticles:
    """A persistent pool of spray particles (ocean_particles, include/oceanfft.h): 8-float records
    (x, y, z, age, velocity x, y, z in m/s, id as the emitter's uint32 bits). One step moves them under gravity
    and drag toward a wind, lands them on the water of a sampler's pairs, compacts survivors and impacts in
    order and appends a SprayEmitter call's records."""

    def __init__(self, fft, capacity: int):
        self.fft = fft
        self.capacity = int(capacity)
        h = ctypes.c_void_p()
        check(lib().ocean_particles_create(ctypes.byref(h), fft.handle, ctypes.c_int64(self.capacity)),
              "ocean_particles_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def step(self, sampler: SurfaceSampler, settings, dt: float, emitter: "SprayEmitter" = None,
             emit_records: int = None, landed: int = None, landed_capacity: int = 0) -> None:
        """Enqueue one step on the plan's stream. settings: an OceanParticleSettings; emitter with emit_records
        (the device pointer its last emit wrote): the records to append, counted by the emitter's device table;
        landed: device rows (landed_capacity, 8) for the impacts, or None to count them only."""
        table = emitter.counts_device() if (emitter is not None and emit_records) else 0
        check(lib().ocean_particles_step(self._h, sampler._gens, sampler._cas, len(sampler.pairs),
                                         ctypes.byref(settings), ctypes.c_float(dt),
                                         ctypes.c_void_p(emit_records or 0), ctypes.c_void_p(table),
                                         ctypes.c_int64(landed_capacity), ctypes.c_void_p(landed or 0)),
              "ocean_particles_step")

    def load(self, records_ptr: int, count: int) -> None:
        """Replace the list with `count` device records (count, 8)."""
        check(lib().ocean_particles_load(self._h, ctypes.c_void_p(records_ptr or 0), ctypes.c_int64(count)),
              "ocean_particles_load")

    def load_host(self, records: np.ndarray) -> None:
        records = np.ascontiguousarray(records).reshape(-1, FLOATS_PER_VERTEX)
        assert records.dtype.itemsize == 4
        src = DeviceBuffer.from_array(records) if records.shape[0] else None
        self.load(src.ptr if src else 0, records.shape[0])
        self.fft.synchronize()  # src is freed on return

    def clear(self) -> None:
        check(lib().ocean_particles_clear(self._h), "ocean_particles_clear")

    @property
    def records_ptr(self) -> int:
        """The current list in device memory: valid until the next step, load or close."""
        ptr = lib().ocean_particles_records(self._h)
        if not ptr:
            raise OceanError(OCEAN_ERR_INVALID, "ocean_particles_records")
        return int(ptr)

    def records_host(self, dtype=np.float32) -> np.ndarray:
        """The live particles (alive, 8) on the host; synchronises the plan's stream."""
        alive = int(self.counts()[0])
        if not alive:
            return np.zeros((0, FLOATS_PER_VERTEX), dtype)
        return hip.to_host(self.records_ptr, (alive, FLOATS_PER_VERTEX), dtype)

    def counts(self) -> np.ndarray:
        """The int64[8] counts on the host; synchronises the plan's stream."""
        out = (ctypes.c_int64 * PARTICLE_COUNTS)()
        check(lib().ocean_particles_counts(self._h, out), "ocean_particles_counts")
        return np.array(out[:], np.int64)

    def counts_device(self) -> int:
        ptr = lib().ocean_particles_counts_device(self._h)
        if not ptr:
            raise OceanError(OCEAN_ERR_INVALID, "ocean_particles_counts_device")
        return int(ptr)

    def close(self) -> None:
        if self._h:
            lib().ocean_particles_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_cascades(pairs):
    """[(height, disp, jac, planeSize, displacement)] host copies, for the CPU oracle."""
    out = []
    for g, c in pairs:
        s = g.GetOceanSettings(c)
        out.append((g.height_map_host(c), g.displacement_map_host(c), g.jacobian_map_host(c), s.planeSize,
                    s.displacement))
    return out


__all__ = ["SurfaceSampler", "HullSet", "SprayEmitter", "SprayParticles", "PARTICLE_ITEM", "host_cascades", "FLOATS_PER_VERTEX", "hip", "camera_pose",
           "default_camera", "default_shading", "default_march", "camera_rays_host", "default_camera_layers",
           "camera_layers_scratch_bytes", "OceanCameraLayers", "DEPOSIT_COUNTS", "DEPOSIT_ITEM"]
