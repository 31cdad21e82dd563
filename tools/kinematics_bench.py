#!/usr/bin/env python3
"""Times ocean_generator_calculate_kinematics and ocean_water_kinematics (depth layers).

calculate_kinematics at 3 x 256^2 (the reference scene, one batched generator), 1 x 4096^2 and 8 x 4096^2 with 1
and 4 depth layers, the legs alternating round by round in one process:
  kinematics  the whole call: the packing kernel and the batched EncodeIFFT of 2 * layers * cascades images
  ifft        that EncodeIFFT alone on the same images; kinematics - ifft is the packing kernel (the method of
              device/k_rates.h's figures)
  copy        ocean_debug_copy of the packing kernel's bytes, 16 + 32 * layers B per point read plus written,
              i.e. a copy of half that, as the streaming yardstick: a packing kernel near it is bound by HBM,
              one well above it by its exponentials
  rates       ocean_generator_calculate_rates of the same generator: by bytes (176 B per point) one layer is one
              calculate_rates
Then ocean_water_kinematics beside ocean_surface_query of the same points (8 iterations, tolerance 0) on 3 x 256^2
cascades with 4 layers, 4096 and 1025^2 points at depths 0 .. 8 m under the surface.
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the median of
ROUNDS windows per leg.

    python tools/kinematics_bench.py [--shapes 3x256,1x4096,8x4096] [--layers 1,4] [--points 4096,1050625]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # noqa: F401  first: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer, hip  # noqa: E402
from oceansimulation_amd.surface import SurfaceSampler  # noqa: E402
from oceansimulation_amd.waves import debug_copy  # noqa: E402

WARMUP, CALLS, ROUNDS = 3, 20, 5
PEAK = 8e12  # B/s
PLANES = (5.0, 17.0, 101.0)
DEPTHS = (0.0, 0.25, 1.0, 4.0)
LAYER_BYTES = 176  # per point and layer: 16 read + 32 written by the packing kernel (h0 once per point), 128 by EncodeIFFT


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


def bench_layers(timer, cascades, n, layers):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
    g.set_depth_layers(DEPTHS[:layers])
    g.CalculateOcean(1.0)
    g.calculate_rates()
    g.calculate_kinematics()
    fft.synchronize()
    points = cascades * n * n
    images = 2 * layers * cascades
    kin_ptr = g.GetKinematicsMap(0, 0, 0)
    pack_bytes = 16 + 32 * layers
    copy_bytes = points * pack_bytes // 2
    src, dst = DeviceBuffer(copy_bytes), DeviceBuffer(copy_bytes)
    wgs = fft.cus * 8
    res = timer.alternating({
        "kinematics": g.calculate_kinematics,
        # the transform alone, on the same images (it overwrites them; the next kinematics leg rewrites them)
        "ifft": lambda: fft.encode_ifft_batch(kin_ptr, images),
        "copy": lambda: debug_copy(dst.ptr, src.ptr, copy_bytes, wgs),
        "rates": g.calculate_rates,
    })
    fft.synchronize()
    k, i, c, r = res["kinematics"], res["ifft"], res["copy"], res["rates"]
    pack = k[0] - i[0]
    total = points * (16 + layers * (LAYER_BYTES - 16))
    print(f"{cascades} x {n}^2, {layers} layer{'s' if layers > 1 else ''}: calculate_kinematics {k[0]:.4f} ms "
          f"({k[1]:.4f}..{k[2]:.4f}; {total / (k[0] * 1e-3) / PEAK:.3f} of 8 TB/s) | its EncodeIFFT of {images} images alone "
          f"{i[0]:.4f} ms ({i[1]:.4f}..{i[2]:.4f}), leaving {pack:.4f} ms for the packing kernel "
          f"({points * pack_bytes / (pack * 1e-3) / PEAK:.3f} of 8 TB/s at {pack_bytes} B/point) | copy of {pack_bytes} B/point "
          f"{c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}): packing = {pack / c[0]:.2f} x the copy | calculate_rates {r[0]:.4f} ms "
          f"({r[1]:.4f}..{r[2]:.4f}): kinematics = {k[0] / (layers * r[0]):.2f} x layers x rates", flush=True)
    src.free()
    dst.free()
    g.close()
    fft.close()


def bench_sampler(timer, counts):
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.set_depth_layers(DEPTHS)
        g.CalculateOcean(1.0)
        g.calculate_kinematics()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    for pts in counts:
        rng = np.random.default_rng(3)
        xz = rng.uniform(-150.0, 150.0, (pts, 2)).astype(np.float32)
        y = -rng.uniform(0.0, 8.0, pts).astype(np.float32)
        xz_dev = DeviceBuffer.from_array(xz)
        xyz_dev = DeviceBuffer.from_array(np.stack([xz[:, 0], y, xz[:, 1]], 1))
        out = DeviceBuffer(pts * 48)
        r = timer.alternating({
            "query": lambda: sampler.query(xz_dev.ptr, pts, 8, 0.0, out.ptr),
            "kinematics": lambda: sampler.kinematics(xyz_dev.ptr, pts, 8, 0.0, out.ptr),
        })
        a, b = r["query"], r["kinematics"]
        print(f"3 x 256^2, 4 layers, {pts} points: surface_query {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}) | "
              f"water_kinematics {b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f}) = {b[0] / a[0]:.2f} x, "
              f"{pts / (b[0] * 1e-3):.3e} points/s", flush=True)
        fft.synchronize()
        for buf in (xz_dev, xyz_dev, out):
            buf.free()
    for g in gens:
        g.close()
    fft.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--layers", default="1,4")
    ap.add_argument("--points", default="4096,1050625")
    args = ap.parse_args()
    timer = Timer()
    print(f"HIP events, median (min..max) of {ROUNDS} alternating windows of {CALLS} calls after {WARMUP} warm-ups")
    for shape in args.shapes.split(","):
        c, n = shape.split("x")
        for layers in args.layers.split(","):
            bench_layers(timer, int(c), int(n), int(layers))
    bench_sampler(timer, [int(p) for p in args.points.split(",")])


if __name__ == "__main__":
    main()
