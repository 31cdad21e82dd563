#!/usr/bin/env python3
"""Times ocean_hulls_step against what a caller had to do before it (hull dynamics).

Three legs on the same device buffers and the same stream, per shape (bodies x points per body) and substeps:
  step           ocean_hulls_step: the loads and the integration of every substep (one launch when every body
                 has at most 64 points, else two per substep)
  loads          ocean_hulls_loads alone, once per substep, the poses left as they are: what integrating costs
                 is the difference to `step`
  loads + torch  ocean_hulls_loads and the same integrator (semi-implicit Euler, Cayley map, one Gram-Schmidt
                 pass) in batched torch ops, once per substep: the route callers write today
The torch leg fuses and orders its arithmetic as torch pleases, so its poses are compared with the fused ones
once, after one call from the same start, as the largest absolute difference.

Every window starts from the same poses (restored outside the timed region) and the bodies then move as they
would in a simulation: dt = 1/60 s per call. Scene, protocol and constants as tools/hulls_bench.py: 3 x 256^2
cascades (planes 5 / 17 / 101 m), 8 iterations, tolerance 0, water velocity on; HIP events on the stream the
legs share, CALLS calls after WARMUP warm-ups per window, the median of ROUNDS windows per leg, the legs
alternating round by round in one process.

    python tools/hulls_step_bench.py [--shapes 4096x16,4096x5,1024x256,1x262144] [--substeps 1,4] [--n 256]
"""
import argparse
import os
import sys

import numpy as np
import torch  # first: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from hulls_bench import CALLS, PLANES, RHO_G, ROUNDS, WARMUP, Timer, random_hull, random_poses  # noqa: E402
from oceansimulation_amd.surface import HullSet, SurfaceSampler  # noqa: E402

DT = 1.0 / 60.0
GRAVITY = (0.0, -9.8, 0.0)


def random_props(rng, points, bodies):
    """Bodies that float: 30 to 80 % of their displaced volume of water as mass, moments of that order."""
    out = np.zeros((bodies, 8), np.float32)
    out[:, 0] = rng.uniform(0.3, 0.8, bodies) * 1000.0 * float(points[:, 3].sum())
    out[:, 1:4] = out[:, :1] * rng.uniform(0.5, 3.0, (bodies, 3))
    out[:, 4:6] = rng.uniform(0.5, 2.0, (bodies, 2))
    return out


class TorchIntegrator:
    """The header's integrator in batched torch ops (every body dynamic, no external wrench)."""

    def __init__(self, props, h):
        self.mass, self.I = props[:, 0:1], props[:, 1:4]
        self.kl, self.ka = 1.0 + h * props[:, 4:5], 1.0 + h * props[:, 5:6]
        self.h = h
        self.g = torch.tensor(GRAVITY, device="cuda")
        self.eye = torch.eye(3, device="cuda")

    def __call__(self, P, loads):
        h = self.h
        R, c, v, w = P[:, :9].reshape(-1, 3, 3), P[:, 9:12], P[:, 12:15], P[:, 15:18]
        v1 = (v + h * (loads[:, 0:3] / self.mass + self.g)) / self.kl
        wb = torch.einsum("nij,ni->nj", R, w)
        tb = torch.einsum("nij,ni->nj", R, loads[:, 4:7])
        wb1 = (wb + h * ((tb - torch.linalg.cross(wb, self.I * wb)) / self.I)) / self.ka
        w1 = torch.einsum("nij,nj->ni", R, wb1)
        a = (0.5 * h) * w1
        n = (a * a).sum(1)[:, None, None]
        z = torch.zeros_like(a[:, 0])
        skew = torch.stack([z, -a[:, 2], a[:, 1], a[:, 2], z, -a[:, 0], -a[:, 1], a[:, 0], z], 1).reshape(-1, 3, 3)
        Q = ((1.0 - n) * self.eye + 2.0 * a[:, :, None] * a[:, None, :] + 2.0 * skew) / (1.0 + n)
        R1 = Q @ R
        e0 = R1[:, 0] / R1[:, 0].norm(dim=1, keepdim=True)
        u = R1[:, 1] - (e0 * R1[:, 1]).sum(1, keepdim=True) * e0
        e1 = u / u.norm(dim=1, keepdim=True)
        P[:, :9] = torch.stack([e0, e1, torch.linalg.cross(e0, e1)], 1).reshape(-1, 9)
        P[:, 9:12] = c + h * v1
        P[:, 12:15] = v1
        P[:, 15:18] = w1


def bench_shape(timer, sampler, bodies, per_body, substeps, iterations):
    rng = np.random.default_rng(bodies)
    points = random_hull(rng, per_body)
    start = torch.as_tensor(random_poses(rng, bodies), device="cuda")
    props_host = random_props(rng, points, bodies)
    props = torch.as_tensor(props_host, device="cuda")
    hulls = HullSet(sampler.fft, points, np.tile(np.array([[0, per_body]], np.int32), (bodies, 1)))
    hulls.set_bodies(props_host)
    settings = HullSet.step_settings(dt=DT, substeps=substeps, gravity=GRAVITY, rho_g=RHO_G, iterations=iterations,
                                     tolerance=0.0, water_velocity=1)
    poses = {name: start.clone() for name in ("step", "loads", "loads + torch")}
    loads = torch.empty((bodies, 8), device="cuda")
    integrate = TorchIntegrator(props, float(np.float32(DT) / np.float32(substeps)))

    def step():
        hulls.step(sampler, poses["step"].data_ptr(), settings)

    def loads_only():
        for _ in range(substeps):
            hulls.loads(sampler, poses["loads"].data_ptr(), loads.data_ptr(), 0, RHO_G, iterations, 0.0, True)

    def loads_torch():
        for _ in range(substeps):
            hulls.loads(sampler, poses["loads + torch"].data_ptr(), loads.data_ptr(), 0, RHO_G, iterations, 0.0, True)
            integrate(poses["loads + torch"], loads)

    legs = {"step": step, "loads": loads_only, "loads + torch": loads_torch}
    step()
    loads_torch()
    torch.cuda.synchronize()
    diff = float((poses["step"] - poses["loads + torch"]).abs().max())
    moved = float((poses["step"] - start).abs().max())
    t = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, call in legs.items():
            poses[name].copy_(start)  # outside the timed region: ms_per_call records its events after the warm-ups
            t[name].append(timer.ms_per_call(call))
    torch.cuda.synchronize()
    r = {name: (sorted(v)[ROUNDS // 2], min(v), max(v)) for name, v in t.items()}
    s, lo, c = r["step"], r["loads"], r["loads + torch"]
    print(f"{bodies} bodies x {per_body} points, {substeps} substeps: ocean_hulls_step {s[0]:.4f} ms ({s[1]:.4f}..{s[2]:.4f}) | "
          f"ocean_hulls_loads alone {lo[0]:.4f} ms ({lo[1]:.4f}..{lo[2]:.4f}): integrating costs {s[0] - lo[0]:+.4f} ms | "
          f"loads + torch integrator {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}) = {c[0] / s[0]:.2f} x | torch poses differ from "
          f"the fused ones by at most {diff:.2e} after one call (the call moves a pose entry by up to {moved:.2e})", flush=True)
    hulls.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x16,4096x5,1024x256,1x262144")
    ap.add_argument("--substeps", default="1,4")
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
          f"velocity on, dt 1/60 s; HIP events, median (min..max) of {ROUNDS} alternating windows of {CALLS} calls after "
          f"{WARMUP} warm-ups")
    for shape in args.shapes.split(","):
        b, p = shape.split("x")
        for substeps in args.substeps.split(","):
            bench_shape(timer, sampler, int(b), int(p), int(substeps), args.iterations)
    for g in gens:
        g.close()
    fft.close()


if __name__ == "__main__":
    main()
