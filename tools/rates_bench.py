#!/usr/bin/env python3
"""Times ocean_generator_calculate_rates and ocean_surface_velocity (rate maps).

calculate_rates at 3 x 256^2 (the reference scene, one batched generator), 1 x 4096^2 and 8 x 4096^2 (the
headline) beside the frame (CalculateOcean) of the same generator, the two legs alternating round by round
in one process. By bytes the rates move 176 B per point (16 read + 32 written by the packing kernel, two
images at EncodeIFFT's 64 B per texel) against the frame's 84. Then ocean_surface_velocity beside
ocean_surface_sample of the same points on 3 x 256^2 cascades, 4096 and 1025^2 points.
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the
median of ROUNDS windows per leg.

    python tools/rates_bench.py [--shapes 3x256,1x4096,8x4096] [--points 4096,1050625]
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

WARMUP, CALLS, ROUNDS = 3, 20, 5
PEAK = 8e12  # B/s
PLANES = (5.0, 17.0, 101.0)
RATE_BYTES, FRAME_BYTES = 176, 84  # per point


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


def bench_rates(timer, cascades, n):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
    g.CalculateOcean(1.0)
    g.calculate_rates()
    fft.synchronize()
    points = cascades * n * n
    rate_ptr = int(ocean.lib().ocean_generator_height_rate_map(g.handle, 0))
    res = timer.alternating({
        "frame": lambda: g.CalculateOcean(1.0 / 60.0),
        "rates": g.calculate_rates,
        # the transform alone, on the same images (it overwrites them; the next rates leg rewrites them)
        "ifft": lambda: fft.encode_ifft_batch(rate_ptr, 2 * cascades),
    })
    fft.synchronize()
    f, r, i = res["frame"], res["rates"], res["ifft"]
    print(f"{cascades} x {n}^2: calculate_rates {r[0]:.4f} ms ({r[1]:.4f}..{r[2]:.4f}; "
          f"{points * RATE_BYTES / (r[0] * 1e-3) / PEAK:.3f} of 8 TB/s at {RATE_BYTES} B/point) | "
          f"frame {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}; {points * FRAME_BYTES / (f[0] * 1e-3) / PEAK:.3f} of 8 TB/s at "
          f"{FRAME_BYTES} B/point) | rates = {r[0] / f[0]:.2f} x the frame (by bytes {RATE_BYTES / FRAME_BYTES:.2f} x) | "
          f"its EncodeIFFT of {2 * cascades} images alone {i[0]:.4f} ms ({i[1]:.4f}..{i[2]:.4f}), leaving "
          f"{r[0] - i[0]:.4f} ms for the packing kernel ({points * 48 / ((r[0] - i[0]) * 1e-3) / PEAK:.3f} of 8 TB/s at 48 B/point)",
          flush=True)
    g.close()
    fft.close()


def bench_velocity(timer, counts):
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.calculate_rates()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    for pts in counts:
        xz = DeviceBuffer.from_array(np.random.default_rng(3).uniform(-150.0, 150.0, (pts, 2)).astype(np.float32))
        out = DeviceBuffer(pts * 32)
        r = timer.alternating({
            "sample": lambda: sampler.sample(xz.ptr, pts, out.ptr),
            "velocity": lambda: sampler.velocity(xz.ptr, pts, out.ptr),
        })
        a, b = r["sample"], r["velocity"]
        print(f"3 x 256^2, {pts} points: surface_sample {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}) | "
              f"surface_velocity {b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f}) = {b[0] / a[0]:.2f} x, "
              f"{pts / (b[0] * 1e-3):.3e} points/s", flush=True)
        fft.synchronize()
        xz.free()
        out.free()
    for g in gens:
        g.close()
    fft.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--points", default="4096,1050625")
    args = ap.parse_args()
    timer = Timer()
    print(f"HIP events, median (min..max) of {ROUNDS} alternating windows of {CALLS} calls after {WARMUP} warm-ups")
    for shape in args.shapes.split(","):
        c, n = shape.split("x")
        bench_rates(timer, int(c), int(n))
    bench_velocity(timer, [int(p) for p in args.points.split(",")])


if __name__ == "__main__":
    main()
