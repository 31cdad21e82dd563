#!/usr/bin/env python3
"""Times ocean_generator_advance_foam and ocean_surface_sample_foam (persistent foam).

The step at 3 x 256^2 (the reference scene, one batched generator), 1 x 4096^2 and 8 x 4096^2, against the
same step composed from torch ops on the exposed device pointers, its three counts included (what a user has
without the call), both legs in one process, alternating round by round. The composed route updates the
library's foam maps in place as the fused one does; before timing, one step of each from zero foam is
compared bit for bit.
The sampler on 3 x 256^2 cascades (three generators on one plan): ocean_surface_sample_foam against
ocean_surface_sample at 4096, 886^2 and 1025^2 random points in +-150 m (between the last two the plain
sample switches to its atlas; the foam sample has none).
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the median
of ROUNDS windows per leg.

    python tools/foam_bench.py [--shapes 3x256,1x4096,8x4096] [--no-sampler]
"""
import argparse
import os
import sys

import numpy as np
import torch  # first: one HIP runtime per process (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import foam_ref as FR  # noqa: E402
import oceansimulation_amd as ocean  # noqa: E402
from mips_bench import PEAK, PLANES, Timer, _DevicePtr  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer  # noqa: E402
from oceansimulation_amd.surface import SurfaceSampler  # noqa: E402

FOAM = dict(bias=1.0, gain=32.0, decay=0.5, level=0.5)
DT = 1.0 / 60.0


def bench_step(timer, cascades, n):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
        ocean.apply_foam_settings(g.GetFoamSettings(c), **FOAM)
    g.CalculateOcean(1.0)
    g.ResetFoam()
    fft.synchronize()
    points = cascades * n * n
    jac = torch.as_tensor(_DevicePtr(g.GetJacobianMap(0), (cascades, n * n)), device="cuda")
    foam = torch.as_tensor(_DevicePtr(g.GetFoamMap(0), (cascades, n * n)), device="cuda")
    a = float(FR.decay_factor(FOAM["decay"], DT))
    launches = 13

    def composed():
        d = FOAM["bias"] - jac                                         # 1
        inj = torch.clamp_min(d, 0.0).mul_(FOAM["gain"]).mul_(DT)      # 2, 3, 4
        t = (foam * a).add_(inj)                                       # 5, 6
        torch.clamp_max(t, 1.0, out=foam)                              # 7
        # three comparisons and three reductions
        return (d > 0).sum(1), (foam >= FOAM["level"]).sum(1), (t >= 1.0).sum(1)

    def fused():
        g.AdvanceFoam(DT)

    fused()
    fft.synchronize()
    lib_map = ocean.hip.to_host(g.GetFoamMap(0), (cascades, n * n))
    lib_counts = np.stack([g.GetFoamCounts(c) for c in range(cascades)])
    g.ResetFoam()
    counts = composed()
    torch.cuda.synchronize()
    same = (np.array_equal(foam.cpu().numpy().view(np.uint32), lib_map.view(np.uint32))
            and np.array_equal(torch.stack(counts, 1).cpu().numpy(), lib_counts))
    res = timer.alternating({"fused": fused, "composed": composed})
    torch.cuda.synchronize()
    f, c = res["fused"], res["composed"]
    frac = points * 12 / (f[0] * 1e-3) / PEAK
    print(f"{cascades} x {n}^2: advance_foam {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}; 2 launches, {frac:.3f} of 8 TB/s at "
          f"12 B/point) | composed from torch {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}; {launches} launches) = "
          f"{c[0] / f[0]:.2f} x | one step from zero equals the composed one: {'yes' if same else 'NO'}", flush=True)
    del jac, foam
    torch.cuda.empty_cache()
    g.close()
    fft.close()
    return f[0] < c[0]


def bench_sampler(timer):
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        ocean.apply_foam_settings(g.GetFoamSettings(0), **FOAM)
        for k in range(8):
            g.CalculateOcean(0.25, k == 0)
            g.AdvanceFoam(0.25)
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    # ocean_surface_sample repacks the maps into its atlas from 2 * 6 * 256^2 = 786432 points on (surface_use_atlas);
    # the foam sampler always samples the maps directly. 886^2 = 784996 is the largest square below that.
    atlas_from = 2 * 2 * len(gens) * 256 * 256
    for points in (4096, 886 * 886, 1025 * 1025):
        xz = np.random.default_rng(5).uniform(-150.0, 150.0, (points, 2)).astype(np.float32)
        src, out = DeviceBuffer.from_array(xz), DeviceBuffer(points * 32)
        res = timer.alternating({"sample": lambda: sampler.sample(src.ptr, points, out.ptr),
                                 "sample_foam": lambda: sampler.sample_foam_device(src.ptr, points, out.ptr)})
        s, f = res["sample"], res["sample_foam"]
        path = "atlas" if points >= atlas_from else "direct"
        print(f"3 x 256^2, {points} points: ocean_surface_sample ({path}) {s[0]:.4f} ms ({s[1]:.4f}..{s[2]:.4f}) | "
              f"ocean_surface_sample_foam (direct) {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) = {f[0] / s[0]:.3f} x "
              f"(the extra taps' share of the loads: 10 dwords per tap and cascade beside 9 = 1.111)", flush=True)
        fft.synchronize()
        src.free()
        out.free()
    for g in gens:
        g.close()
    fft.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--no-sampler", action="store_true")
    args = ap.parse_args()
    timer = Timer()
    print("HIP events, median (min..max) of 5 alternating windows of 20 calls after 3 warm-ups")
    ok = True
    for shape in args.shapes.split(","):
        c, n = shape.split("x")
        ok = bench_step(timer, int(c), int(n)) and ok
    print("advance_foam faster than the composed step at every shape: " + ("yes" if ok else "NO"), flush=True)
    if not args.no_sampler:
        bench_sampler(timer)


if __name__ == "__main__":
    main()
