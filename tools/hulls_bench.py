#!/usr/bin/env python3
"""Times ocean_hulls_loads against the route a caller had to take before it (hull sets).

The fused call: poses in, one wrench per body out (point_out off). The composed route, on the same device
buffers and the same stream: a torch pose transform, ocean_surface_query, a gather of slots 0 and 2,
ocean_surface_velocity, the load arithmetic in torch and a per-body index_add_ (float atomics: its sums
differ from run to run in the last bits, so the two routes are compared with a tolerance, once, before the
timing). The per-instance hull points and body indices of the composed route are gathered once outside the
timed windows (they do not change from step to step).

Scene: 3 x 256^2 cascades (planes 5 / 17 / 101 m), 8 iterations, tolerance 0, water velocity on. Shapes:
bodies x points per body. HIP events on the (default) stream both legs share, CALLS calls after WARMUP
warm-ups per window, the median of ROUNDS windows per leg, the legs alternating round by round in one process.

Shapes of at most 32 points per body also time the same set with the packing of small bodies switched off
(ocean_debug_hulls_packing): every body on a wave of its own.

    python tools/hulls_bench.py [--shapes 4096x16,4096x5,1024x256,1x262144] [--n 256] [--iterations 8]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # first: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from oceansimulation_amd.hip import hip  # noqa: E402
from oceansimulation_amd.surface import HullSet, SurfaceSampler  # noqa: E402

WARMUP, CALLS, ROUNDS = 3, 20, 7
PLANES = (5.0, 17.0, 101.0)
RHO_G = 9810.0


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


def random_hull(rng, n):
    pts = np.zeros((n, 8), np.float32)
    pts[:, 0:3] = rng.uniform(-1.0, 1.0, (n, 3)) * (2.0, 0.6, 4.0)
    pts[:, 3] = rng.uniform(0.01, 0.1, n)
    pts[:, 4] = rng.uniform(0.05, 0.3, n)
    pts[:, 5] = rng.uniform(0.0, 50.0, n)
    pts[:, 6] = rng.uniform(0.0, 20.0, n)
    return pts


def random_poses(rng, bodies):
    out = np.zeros((bodies, 20), np.float32)
    q, r = np.linalg.qr(rng.standard_normal((bodies, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    out[:, :9] = q.reshape(bodies, 9)
    out[:, 9], out[:, 10], out[:, 11] = rng.uniform(-150, 150, bodies), rng.uniform(-0.6, 0.6, bodies), rng.uniform(-150, 150, bodies)
    out[:, 12:15] = rng.uniform(-2.0, 2.0, (bodies, 3))
    out[:, 15:18] = rng.uniform(-0.5, 0.5, (bodies, 3))
    return out


class Composed:
    """The route without ocean_hulls_loads, buffers allocated once."""

    def __init__(self, sampler, points, bodies, per_body, poses, iterations):
        self.sampler, self.iterations = sampler, iterations
        self.n = bodies * per_body
        self.L = torch.as_tensor(np.tile(points, (bodies, 1)), device="cuda")  # per instance point
        self.body = torch.arange(bodies, device="cuda").repeat_interleave(per_body)
        self.poses = poses
        self.xz = torch.empty((self.n, 2), device="cuda")
        self.q = torch.empty((self.n, 8), device="cuda")
        self.base = torch.empty((self.n, 2), device="cuda")
        self.vel = torch.empty((self.n, 8), device="cuda")
        self.loads = torch.empty((bodies, 8), device="cuda")

    def __call__(self):
        P = self.poses[self.body]
        L = self.L
        d = torch.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), L[:, :3])
        x = P[:, 9:12] + d
        self.xz.copy_(x[:, [0, 2]])
        self.sampler.query(self.xz.data_ptr(), self.n, self.iterations, 0.0, self.q.data_ptr())
        self.base.copy_(self.q[:, [0, 2]])
        self.sampler.velocity(self.base.data_ptr(), self.n, self.vel.data_ptr())
        s = ((self.q[:, 1] - x[:, 1]) / (L[:, 4] + L[:, 4]) + 0.5).clamp(0.0, 1.0)
        rel = self.vel[:, 4:7] - (P[:, 12:15] + torch.linalg.cross(P[:, 15:18], d))
        k = s * (L[:, 5] + L[:, 6] * rel.norm(dim=1))
        vs = L[:, 3] * s
        F = k[:, None] * rel
        F[:, 1] += RHO_G * vs
        a = torch.cat([F, vs[:, None], torch.linalg.cross(d, F), (s > 0).float()[:, None]], dim=1)
        self.loads.zero_()
        self.loads.index_add_(0, self.body, a)
        return self.loads


def bench_shape(timer, sampler, bodies, per_body, iterations):
    rng = np.random.default_rng(bodies)
    points = random_hull(rng, per_body)
    poses = torch.as_tensor(random_poses(rng, bodies), device="cuda")
    hulls = HullSet(sampler.fft, points, np.tile(np.array([[0, per_body]], np.int32), (bodies, 1)))
    loads = torch.empty((bodies, 8), device="cuda")
    composed = Composed(sampler, points, bodies, per_body, poses, iterations)

    def fused():
        hulls.loads(sampler, poses.data_ptr(), loads.data_ptr(), 0, RHO_G, iterations, 0.0, True)

    fused()
    ref = composed()
    torch.cuda.synchronize()
    scale = ref.abs().amax(dim=0).clamp_min(1e-30)
    diff = float(((loads - ref).abs().amax(dim=0) / scale).max())
    legs = {"fused": fused, "composed": composed}
    if per_body <= 32:  # the same set with every body on its own waves (no packing of small bodies)
        ocean.lib().ocean_debug_hulls_packing(0)
        own = HullSet(sampler.fft, points, np.tile(np.array([[0, per_body]], np.int32), (bodies, 1)))
        ocean.lib().ocean_debug_hulls_packing(1)
        legs["own waves"] = lambda: own.loads(sampler, poses.data_ptr(), loads.data_ptr(), 0, RHO_G, iterations, 0.0, True)
    r = timer.alternating(legs)
    torch.cuda.synchronize()
    f, c = r["fused"], r["composed"]
    if "own waves" in r:
        o = r["own waves"]
        print(f"{bodies} bodies x {per_body} points: bodies sharing waves {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) | every body "
              f"on its own wave {o[0]:.4f} ms ({o[1]:.4f}..{o[2]:.4f}) = {o[0] / f[0]:.2f} x", flush=True)
    print(f"{bodies} bodies x {per_body} points ({bodies * per_body} instance points): ocean_hulls_loads {f[0]:.4f} ms "
          f"({f[1]:.4f}..{f[2]:.4f}) | composed route {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}) = {c[0] / f[0]:.2f} x | "
          f"{bodies * per_body / (f[0] * 1e-3):.3e} points/s fused | worst component difference between the routes "
          f"{diff:.2e} of the component's max", flush=True)
    hulls.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x16,4096x5,1024x256,1x262144")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=8)
    args = ap.parse_args()
    timer = Timer()
    fft = ocean.FFTCalculator(args.n)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.calculate_rates()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    print(f"{torch.cuda.get_device_name(0)}; 3 x {args.n}^2 cascades, {args.iterations} iterations, tolerance 0, water "
          f"velocity on; HIP events, median (min..max) of {ROUNDS} alternating windows of {CALLS} calls after {WARMUP} "
          f"warm-ups")
    for shape in args.shapes.split(","):
        b, p = shape.split("x")
        bench_shape(timer, sampler, int(b), int(p), args.iterations)
    for g in gens:
        g.close()
    fft.close()


if __name__ == "__main__":
    main()
