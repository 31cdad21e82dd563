#!/usr/bin/env python3
"""Times ocean_generator_build_mips and the LOD plane sampling (mip pyramids).

build_mips at 3 x 256^2 (the reference scene, one batched generator), 1 x 4096^2 and 8 x 4096^2 (the
headline), against two baselines in the same process, the legs alternating round by round:
  per level  the same pyramid built level by level with torch.nn.functional.avg_pool2d reading the same
             device buffers (the maps wrapped as channels-last tensors: heightMap and displacementMap as
             one batch, the Jacobian as another, so 2 launches per level)
  copy       ocean_debug_copy of the build's algorithmic bytes, 48 B per point (36 read + 12 written),
             i.e. a copy of 24 B per point, as the streaming yardstick
Then ocean_surface_sample_plane_lod against ocean_surface_sample_plane on 3 x 256^2 at res 1024 and 4096.
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the
median of ROUNDS windows per leg.

    python tools/mips_bench.py [--shapes 3x256,1x4096,8x4096] [--plane-res 1024,4096]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # first: one HIP runtime per process (tests/conftest.py)
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer, hip  # noqa: E402
from oceansimulation_amd.surface import SurfaceSampler  # noqa: E402
from oceansimulation_amd.waves import debug_copy  # noqa: E402

WARMUP, CALLS, ROUNDS = 3, 20, 5
PEAK = 8e12  # B/s
PLANES = (5.0, 17.0, 101.0)


def _hip_ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")


class Timer:
    def __init__(self):
        self.h, self.stream = hip(), ctypes.c_void_p(0)
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for f in (self.h.hipEventCreate, self.h.hipEventRecord, self.h.hipEventSynchronize, self.h.hipEventElapsedTime):
            f.restype = ctypes.c_int
        self.h.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.h.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.h.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        _hip_ok(self.h.hipEventCreate(ctypes.byref(self.a)), "hipEventCreate")
        _hip_ok(self.h.hipEventCreate(ctypes.byref(self.b)), "hipEventCreate")

    def ms_per_call(self, call):
        for _ in range(WARMUP):
            call()
        _hip_ok(self.h.hipEventRecord(self.a, self.stream), "hipEventRecord")
        for _ in range(CALLS):
            call()
        _hip_ok(self.h.hipEventRecord(self.b, self.stream), "hipEventRecord")
        _hip_ok(self.h.hipEventSynchronize(self.b), "hipEventSynchronize")
        ms = ctypes.c_float()
        _hip_ok(self.h.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b), "hipEventElapsedTime")
        return ms.value / CALLS

    def alternating(self, legs):
        """legs: {name: call}. One window of every leg per round; per leg (median, min, max) ms."""
        t = {name: [] for name in legs}
        for _ in range(ROUNDS):
            for name, call in legs.items():
                t[name].append(self.ms_per_call(call))
        return {name: (sorted(v)[ROUNDS // 2], min(v), max(v)) for name, v in t.items()}


class _DevicePtr:
    """A device buffer of the library seen by torch (no copy)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def bench_build(timer, cascades, n):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
    g.CalculateOcean(1.0)
    g.build_mips()
    fft.synchronize()
    top = n.bit_length() - 1
    points = cascades * n * n
    # the maps: [cascade][heightMap, displacementMap][n][n] float4 and [cascade][n][n] float
    hd = torch.as_tensor(_DevicePtr(g.GetHeightMap(0), (2 * cascades, n, n, 4)), device="cuda").permute(0, 3, 1, 2)
    jac = torch.as_tensor(_DevicePtr(g.GetJacobianMap(0), (cascades, 1, n, n)), device="cuda")

    def per_level():
        a, b = hd, jac
        for _ in range(top):
            a, b = TF.avg_pool2d(a, 2), TF.avg_pool2d(b, 2)
        return a, b

    # the torch pyramid reads what the kernel reads: its top level is the library's within fp32 rounding
    a, _ = per_level()
    torch.cuda.synchronize()
    lib_top = g.height_mip_host(0, top).reshape(4)
    err = float(np.max(np.abs(a[0].reshape(4).cpu().numpy() - lib_top)))
    copy_bytes = points * 24
    src, dst = DeviceBuffer(copy_bytes), DeviceBuffer(copy_bytes)
    wgs = fft.cus * 8
    res = timer.alternating({
        "fused": g.build_mips,
        "per level": per_level,
        "copy": lambda: debug_copy(dst.ptr, src.ptr, copy_bytes, wgs),
    })
    torch.cuda.synchronize()
    f, p, c = res["fused"], res["per level"], res["copy"]
    frac = points * 48 / (f[0] * 1e-3) / PEAK
    launches = (top + 5) // 6
    print(f"{cascades} x {n}^2: fused {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}; {launches} launches, {frac:.3f} of 8 TB/s at 48 B/point) | "
          f"per level {p[0]:.4f} ms ({p[1]:.4f}..{p[2]:.4f}; {2 * top} launches) = {p[0] / f[0]:.2f} x fused | "
          f"copy of 48 B/point {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}) = {c[0] / f[0]:.2f} x fused | "
          f"top level, torch against the library: {err:.2e}", flush=True)
    ok = f[0] <= p[0]
    print(f"    fused no slower than per level: {'yes' if ok else 'NO'}", flush=True)
    src.free()
    dst.free()
    del hd, jac, a
    torch.cuda.empty_cache()
    g.close()
    fft.close()
    return ok


def bench_plane(timer, resolutions):
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.build_mips()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    cam = [0.0, 5.0, 0.0, -0.70711, 0.70711]
    for res in resolutions:
        out = DeviceBuffer((res + 1) * (res + 1) * 32)
        r = timer.alternating({
            "plane": lambda: sampler.sample_plane(cam, res, out.ptr),
            "plane lod": lambda: sampler.sample_plane_lod(cam, res, out.ptr),
        })
        a, b = r["plane"], r["plane lod"]
        print(f"3 x 256^2, plane mesh res {res} ({(res + 1) ** 2} vertices): sample_plane {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}) | "
              f"sample_plane_lod {b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f}) = {b[0] / a[0]:.2f} x", flush=True)
        fft.synchronize()
        out.free()
    for g in gens:
        g.close()
    fft.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--plane-res", default="1024,4096")
    args = ap.parse_args()
    timer = Timer()
    print(f"HIP events, median (min..max) of {ROUNDS} alternating windows of {CALLS} calls after {WARMUP} warm-ups")
    ok = True
    for shape in args.shapes.split(","):
        c, n = shape.split("x")
        ok = bench_build(timer, int(c), int(n)) and ok
    bench_plane(timer, [int(r) for r in args.plane_res.split(",")])
    print("build_mips no slower than the per-level baseline at every shape: " + ("yes" if ok else "NO"))


if __name__ == "__main__":
    main()
