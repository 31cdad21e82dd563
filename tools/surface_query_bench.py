#!/usr/bin/env python3
"""Times ocean_surface_query against ocean_surface_sample on the same points (surface
consumer): the 3 x 256^2 scene at t = 1, positions uniform in a +-400 m box, HIP events on the plan's
stream around 20 calls after 3 warm-ups, the median of 5 such windows (and their spread). The path
columns restate surface_use_atlas / surface_query_use_atlas (launch_surface.hip): which of the maps or
the repacked atlas each call samples.

    python tools/surface_query_bench.py [--n 256] [--points 4096,1050625] [--iterations 8] [--steep]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer, hip  # noqa: E402
from oceansimulation_amd.surface import SurfaceSampler  # noqa: E402

WARMUP, CALLS, ROUNDS = 3, 20, 5


def _hip_ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")


class Timer:
    def __init__(self, stream):
        self.h, self.stream = hip(), ctypes.c_void_p(stream)
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

    def median_ms(self, call):
        """(median, min, max) of ROUNDS windows of CALLS calls each."""
        t = sorted(self.ms_per_call(call) for _ in range(ROUNDS))
        return t[ROUNDS // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--points", default="4096,16384,65536,196608,393216,786432,1050625")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--steep", action="store_true", help="displacement = 1, scale = 2 (folded crests)")
    args = ap.parse_args()

    h = hip()
    h.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    h.hipStreamCreate.restype = ctypes.c_int
    stream = ctypes.c_void_p()
    _hip_ok(h.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
    fft = ocean.FFTCalculator(args.n, stream.value)
    gens = []
    for L in (5.0, 17.0, 101.0):
        g = ocean.Generator(fft, 1)
        extra = dict(displacement=1.0, scale=2.0) if args.steep else {}
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L, **extra)
        g.CalculateOcean(1.0)
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    timer = Timer(stream.value)
    counts = [int(c) for c in args.points.split(",")]
    xz_all = np.random.default_rng(11).uniform(-400.0, 400.0, (max(counts), 2)).astype(np.float32)
    src = DeviceBuffer.from_array(xz_all)
    out = DeviceBuffer(max(counts) * 32)
    texels = 2 * 3 * args.n * args.n  # surface_atlas_texels
    fits = texels * 16 <= 256 << 20
    q_floor, q_share = (16384, 96) if args.iterations >= 2 else (65536, 48)
    print(f"scene 3 x {args.n}^2{' steep' if args.steep else ''}, box +-400 m, {args.iterations} iterations, HIP events, median of {ROUNDS} x "
          f"({CALLS} calls after {WARMUP} warm-ups)")
    print(f"{'points':>9} {'sample':>6} {'query':>6} {'sample ms':>10} {'query tol 0':>12} {'query 1e-4':>11} {'ratio 0':>8} {'ratio 1e-4':>10}")
    for pts in counts:
        path = "atlas" if fits and pts >= 65536 and pts >= 2 * texels else "direct"
        qpath = "atlas" if fits and pts >= q_floor and pts * q_share >= texels else "direct"
        s3 = timer.median_ms(lambda: sampler.sample(src.ptr, pts, out.ptr))
        q3 = timer.median_ms(lambda: sampler.query(src.ptr, pts, args.iterations, 0.0, out.ptr))
        r3 = timer.median_ms(lambda: sampler.query(src.ptr, pts, args.iterations, 1e-4, out.ptr))
        t_s, t_q0, t_q4 = s3[0], q3[0], r3[0]
        spread = max((m[2] - m[1]) / m[0] for m in (s3, q3, r3))
        print(f"{pts:9d} {path:>6} {qpath:>6} {t_s:10.4f} {t_q0:12.4f} {t_q4:11.4f} {t_q0 / t_s:8.2f} {t_q4 / t_s:10.2f}"
              f"   (max - min within {100 * spread:.0f} % of the median)", flush=True)
    fft.synchronize()


if __name__ == "__main__":
    main()
