#!/usr/bin/env python3
"""Times ocean_generator_build_bounds and ocean_surface_raycast (bounds and ray casting).

Bounds at 3 x 256^2 (the reference scene, one batched generator), 1 x 4096^2 and 8 x 4096^2, against two
legs in the same process, alternating round by round:
  aminmax  torch.aminmax over the same nine channels reading the same device buffers (the composed route:
           one reduction for heightMap + displacementMap, one for the Jacobian)
  mips     ocean_generator_build_mips: the same 36 B per point read, plus 12 B written
Raycast on 3 x 256^2 cascades (step 0.25, 256 steps, 10 bisections, 4 iterations, tolerance 1e-3, pad 0),
a 64 x 1024 lidar fan (depression 1-30 degrees) and 1025^2 camera rays from 10 m, fixed steps and slope 1,
against the composed route: per marching step a torch kernel advances the rays, one ocean_surface_query
launch runs on all rays, and torch compares and masks; it takes the step count of the fused call's slowest
ray and does no bisection, so it does less work per ray than the fused call. Mean fixed-point steps per ray
come from tests/raycast_ref.py on every 64th ray (the kernel does not count them).
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the median
of ROUNDS windows per leg.

    python tools/raycast_bench.py [--shapes 3x256,1x4096,8x4096] [--no-rays]
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

import oceansimulation_amd as ocean  # noqa: E402
from mips_bench import PEAK, PLANES, Timer, _DevicePtr  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer  # noqa: E402
from oceansimulation_amd.surface import SurfaceSampler, host_cascades  # noqa: E402

PARAMS = dict(step=0.25, max_steps=256, refine=10, iterations=4, tolerance=1e-3, pad=0.0)


def bench_bounds(timer, cascades, n):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
    g.CalculateOcean(1.0)
    g.build_mips()
    g.BuildBounds()
    fft.synchronize()
    points = cascades * n * n
    hd = torch.as_tensor(_DevicePtr(g.GetHeightMap(0), (cascades, 2, n * n, 4)), device="cuda")
    jac = torch.as_tensor(_DevicePtr(g.GetJacobianMap(0), (cascades, n * n)), device="cuda")

    def aminmax():
        return torch.aminmax(hd, dim=2), torch.aminmax(jac, dim=1)

    (lo, hi), (jlo, jhi) = aminmax()
    torch.cuda.synchronize()
    want = np.zeros((cascades, 9, 2), np.float32)
    want[:, :8, 0], want[:, :8, 1] = lo.reshape(cascades, 8).cpu().numpy(), hi.reshape(cascades, 8).cpu().numpy()
    want[:, 8, 0], want[:, 8, 1] = jlo.cpu().numpy(), jhi.cpu().numpy()
    same = all(np.array_equal(g.GetBounds(c), want[c]) for c in range(cascades))
    res = timer.alternating({"bounds": g.BuildBounds, "aminmax": aminmax, "mips": g.build_mips})
    torch.cuda.synchronize()
    b, a, m = res["bounds"], res["aminmax"], res["mips"]
    frac = points * 36 / (b[0] * 1e-3) / PEAK
    print(f"{cascades} x {n}^2: build_bounds {b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f}; 2 launches, {frac:.3f} of 8 TB/s at "
          f"36 B/point) | torch.aminmax {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}; 2 reductions) = {a[0] / b[0]:.2f} x | "
          f"build_mips {m[0]:.4f} ms ({m[1]:.4f}..{m[2]:.4f}) = {m[0] / b[0]:.2f} x | equals torch.aminmax: "
          f"{'yes' if same else 'NO'}", flush=True)
    print(f"    bounds no slower than the mips build: {'yes' if b[0] <= m[0] else 'NO'}", flush=True)
    del hd, jac
    torch.cuda.empty_cache()
    g.close()
    fft.close()
    return b[0] <= m[0]


def fan_rays():
    """64 rings x 1024 azimuths from a mast at (0, 10, 0), depression 1 .. 30 degrees."""
    dep = np.radians(np.linspace(1.0, 30.0, 64))[:, None]
    az = (2.0 * np.pi * np.arange(1024) / 1024)[None, :]
    rays = np.zeros((64, 1024, 8), np.float32)
    rays[..., 1], rays[..., 7] = 10.0, 400.0
    rays[..., 4], rays[..., 5], rays[..., 6] = np.cos(dep) * np.cos(az), -np.sin(dep) * np.ones_like(az), np.cos(dep) * np.sin(az)
    return rays.reshape(-1, 8)


def camera_rays(res=1025):
    """A pinhole camera at (0, 10, 0) looking along +x, 20 degrees down, 60 degrees field of view."""
    s = np.tan(np.radians(30.0)) * np.linspace(-1.0, 1.0, res)
    u, v = np.meshgrid(s, s)
    pitch = np.radians(20.0)
    fwd = np.array([np.cos(pitch), -np.sin(pitch), 0.0])
    up = np.array([np.sin(pitch), np.cos(pitch), 0.0])
    right = np.array([0.0, 0.0, 1.0])
    d = fwd[None, None] + u[..., None] * right + v[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((res, res, 8), np.float32)
    rays[..., 1], rays[..., 7] = 10.0, 400.0
    rays[..., 4:7] = d
    return rays.reshape(-1, 8)


def bench_rays(timer):
    from oracle import oracle as O

    import raycast_ref as RR

    O.build()
    O.set_threads(min(16, os.cpu_count() or 1))
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.BuildBounds()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    host = host_cascades(sampler.pairs)
    for name, rays in (("lidar fan 64 x 1024", fan_rays()), ("camera 1025^2", camera_rays())):
        n = rays.shape[0]
        src, out = DeviceBuffer.from_array(rays), DeviceBuffer(n * 64)
        r = torch.as_tensor(_DevicePtr(src.ptr, (n, 8)), device="cuda")
        xz = torch.empty((n, 2), device="cuda")
        qout = torch.empty((n, 8), device="cuda")
        for slope in (float("inf"), 1.0):
            sampler.raycast(src.ptr, n, out.ptr, slope=slope, **PARAMS)
            fft.synchronize()
            hits = out.to_host((n, 16))
            steps = int(hits[:, 14].max())
            sub = rays[::64].copy()
            _, stats = RR.raycast(O, host, sub, slope=slope, with_stats=True, **PARAMS)

            def composed():
                t = r[:, 3].clone()
                alive = torch.ones(n, dtype=torch.bool, device="cuda")
                t_hit = torch.zeros(n, device="cuda")
                below = None
                for _ in range(steps + 1):
                    torch.stack((r[:, 0] + t * r[:, 4], r[:, 2] + t * r[:, 6]), 1, out=xz)
                    sampler.query(xz.data_ptr(), n, PARAMS["iterations"], PARAMS["tolerance"], qout.data_ptr())
                    neg = (r[:, 1] + t * r[:, 5]) - qout[:, 1] <= 0
                    if below is None:
                        below = neg
                    cross = alive & (neg != below)
                    t_hit = torch.where(cross, t, t_hit)
                    alive = alive & ~cross
                    t = torch.where(alive, t + PARAMS["step"], t)
                return t_hit

            res = timer.alternating({"fused": lambda: sampler.raycast(src.ptr, n, out.ptr, slope=slope, **PARAMS),
                                     "composed": composed})
            torch.cuda.synchronize()
            f, c = res["fused"], res["composed"]
            counts = np.bincount(hits[:, 12].astype(int), minlength=4).tolist()
            print(f"3 x 256^2, {name} ({n} rays), slope {slope}: fused {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) = "
                  f"{n / (f[0] * 1e-3):.3e} rays/s | composed, {steps} steps {c[0]:.3f} ms ({c[1]:.3f}..{c[2]:.3f}) = "
                  f"{c[0] / f[0]:.1f} x fused | HIT/OUTSIDE/EXIT/STEP_LIMIT {counts} | mean steps per ray "
                  f"{hits[:, 14].mean():.1f}, evaluations {stats['evals'] / len(sub):.1f} and fixed-point steps "
                  f"{stats['fp_steps'] / len(sub):.1f} per ray (reference, every 64th ray)", flush=True)
        fft.synchronize()
        src.free()
        out.free()
    for g in gens:
        g.close()
    fft.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--no-rays", action="store_true")
    args = ap.parse_args()
    timer = Timer()
    print("HIP events, median (min..max) of 5 alternating windows of 20 calls after 3 warm-ups")
    ok = True
    for shape in args.shapes.split(","):
        c, n = shape.split("x")
        ok = bench_bounds(timer, int(c), int(n)) and ok
    print("build_bounds no slower than build_mips at every shape: " + ("yes" if ok else "NO"), flush=True)
    if not args.no_rays:
        bench_rays(timer)


if __name__ == "__main__":
    main()
