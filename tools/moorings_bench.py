#!/usr/bin/env python3
"""Times ocean_moorings_step against the route a caller had to take before it (mooring lines).

The fused call: two launches whatever `substeps` is (the lines' kernel and the per-body sum). The composed
route, on the same stream: per substep one ocean_water_kinematics over all nodes (water 1 only) and the step's
arithmetic in torch on (lines, nodes) tensors, a few dozen small launches. Both start from the same reset nodes;
the composed route's nodes are compared with the fused call's once, before the timing (torch orders and fuses its
norms and sums its own way, so a difference of a few float32 ulps of the positions is printed, not 0). The timed calls run on from
wherever the nodes are: the lines stay within a few metres, and the work per call does not depend on the state
(water 0), or only through the query's iterations, which are fixed (tolerance 0).

Shapes: lines x nodes per line, every line on a body of its own (one pose per line), anchors 30 m down and
12 m off. Lines of at most 32 nodes also time the same set with the packing switched off
(ocean_debug_hulls_packing): every line on a wave of its own.

HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the median of
ROUNDS windows per leg, the legs alternating round by round in one process.

    python tools/moorings_bench.py [--shapes 4096x8,1024x64,1x64] [--substeps 1,8,64] [--n 256] > profiles/moorings_bench.log
"""
import argparse
import os
import sys

import numpy as np
import torch  # first: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oceansimulation_amd as ocean  # noqa: E402
from hulls_bench import PLANES, RHO_G, Timer, random_poses  # noqa: E402
from oceansimulation_amd.surface import MooringSet, SurfaceSampler  # noqa: E402

DEPTHS = (0.0, 0.5, 2.0, 8.0)
DT = 1.0 / 60.0
BED = dict(bed_y=-28.0, bed_k=2e4, bed_c=200.0)
GRAVITY = (0.0, -9.8, 0.0)


def make_lines(rng, poses, count, nodes):
    lines = np.zeros((count, 16), np.float32)
    lf = rng.uniform(-1.0, 1.0, (count, 3)) * (2.0, 0.5, 4.0)
    top = poses[:, 9:12] + np.einsum("nij,nj->ni", poses[:, :9].reshape(-1, 3, 3), lf)
    a = rng.uniform(0.0, 2.0 * np.pi, count)
    anchor = top + np.stack([12.0 * np.cos(a), np.zeros(count), 12.0 * np.sin(a)], -1)
    anchor[:, 1] = -30.0
    lines[:, 0:3], lines[:, 3:6] = anchor, lf
    lines[:, 6] = np.linalg.norm(top - anchor, axis=1) * 1.02
    # EA / mass_per_m low enough for h = dt / 1 at every node count timed: h < l0 sqrt(mass_per_m / EA)
    lines[:, 7], lines[:, 8], lines[:, 9] = 2e3, 20.0, 8.0
    lines[:, 10], lines[:, 11], lines[:, 12] = 2e-3, 3.0, 2.0
    attach = np.stack([np.arange(count), np.full(count, nodes)], -1).astype(np.int32)
    return lines, attach


class Composed:
    """One call without ocean_moorings_step: `substeps` times ocean_water_kinematics and the arithmetic in torch."""

    def __init__(self, sampler, lines, attach, poses, nodes, substeps, water):
        dev = "cuda"
        self.sampler, self.substeps, self.water = sampler, substeps, water
        L = torch.as_tensor(lines, device=dev)
        n = int(attach[0, 1])
        self.count, self.n = lines.shape[0], n
        l0 = L[:, 6] / float(n - 1)
        self.l0, self.ea, self.ca = l0[:, None], L[:, 7:8], L[:, 8:9]
        self.mn, self.vn, self.dl, self.dq = (L[:, 9:10] * self.l0, L[:, 10:11] * self.l0, L[:, 11:12] * self.l0,
                                              L[:, 12:13] * self.l0)
        self.kb, self.cb = BED["bed_k"] * self.l0, BED["bed_c"] * self.l0
        self.h = float(np.float32(DT) / np.float32(substeps))
        P = torch.as_tensor(poses, device=dev)
        d = torch.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), L[:, 3:6])
        self.P, self.vp = P[:, 9:12] + d, P[:, 12:15] + torch.linalg.cross(P[:, 15:18], d)
        self.A = L[:, 0:3]
        N = torch.as_tensor(nodes, device=dev).reshape(self.count, n, 8)
        self.x, self.v = N[:, :, 0:3].clone(), N[:, :, 4:7].clone()
        self.g = torch.tensor(GRAVITY, device=dev)
        self.xyz = torch.empty((self.count * n, 3), device=dev)
        self.kin = torch.empty((self.count * n, 12), device=dev)
        self.fm = torch.zeros((self.count, 3), device=dev)

    def __call__(self):
        x, v, h = self.x, self.v, self.h
        x[:, 0], v[:, 0] = self.A, 0.0
        x[:, -1], v[:, -1] = self.P, self.vp
        total = torch.zeros_like(self.fm)
        for _ in range(self.substeps):
            dv = x[:, 1:] - x[:, :-1]
            ln = dv.norm(dim=2)
            e = torch.where(ln[..., None] > 0, dv / ln[..., None], torch.zeros_like(dv))
            rate = ((v[:, 1:] - v[:, :-1]) * e).sum(2) / self.l0
            T = (self.ea * ((ln - self.l0) / self.l0) + self.ca * rate).clamp_min(0.0)
            S = T[..., None] * e
            total = total - S[:, -1]
            xi, vi = x[:, 1:-1], v[:, 1:-1]
            if self.water:
                self.xyz.copy_(x.reshape(-1, 3))
                self.sampler.kinematics(self.xyz.data_ptr(), self.xyz.shape[0], 4, 0.0, self.kin.data_ptr())
                kin = self.kin.reshape(self.count, self.n, 12)[:, 1:-1]
                u, wet = kin[:, :, 4:7], kin[:, :, 11] != 0
            else:
                u, wet = torch.zeros_like(vi), (0.0 - xi[:, :, 1]) > 0
            rel = u - vi
            k = torch.where(wet, self.dl + self.dq * rel.norm(dim=2), torch.zeros_like(ln[:, 1:]))
            Fo = ((S[:, 1:] - S[:, :-1]) + k[..., None] * rel) + self.mn[..., None] * self.g
            Fo[:, :, 1] += torch.where(wet, RHO_G * self.vn, torch.zeros_like(k))
            pen = BED["bed_y"] - xi[:, :, 1]
            bed = pen > 0
            Fo[:, :, 1] += torch.where(bed, self.kb * pen, torch.zeros_like(pen))
            Fo -= torch.where(bed[..., None], self.cb[..., None] * vi, torch.zeros_like(vi))
            vi += h * (Fo / self.mn[..., None])
            xi += h * vi
        self.fm = total / float(self.substeps)
        return x


def bench_shape(timer, sampler, count, nodes, substeps, water):
    rng = np.random.default_rng(count * 64 + nodes)
    poses = random_poses(rng, count)
    lines, attach = make_lines(rng, poses, count, nodes)
    dposes = torch.as_tensor(poses, device="cuda")
    wrench = torch.empty((count, 8), device="cuda")
    kw = dict(dt=DT, substeps=substeps, rho_g=RHO_G, water=water, iterations=4, tolerance=0.0, **BED)
    settings = MooringSet.settings(**kw)
    moorings = MooringSet(sampler.fft, lines, attach, count)
    moorings.reset(dposes.data_ptr())
    start = moorings.nodes_host()
    composed = Composed(sampler, lines, attach, poses, start, substeps, water)

    def fused(m=moorings):
        m.step(sampler if water else None, dposes.data_ptr(), wrench.data_ptr(), 0, settings)

    fused()
    ref = composed()
    torch.cuda.synchronize()
    got = torch.as_tensor(moorings.nodes_host(), device="cuda").reshape(count, nodes, 8)[:, :, 0:3]
    diff = float((got - ref).abs().max())
    legs = {"fused": fused, "composed": composed}
    if nodes <= 32:
        ocean.lib().ocean_debug_hulls_packing(0)
        own = MooringSet(sampler.fft, lines, attach, count)
        ocean.lib().ocean_debug_hulls_packing(1)
        own.reset(dposes.data_ptr())
        legs["own waves"] = lambda: fused(own)
    r = timer.alternating(legs)
    torch.cuda.synchronize()
    f, c = r["fused"], r["composed"]
    head = f"{count} lines x {nodes} nodes, water {water}, {substeps} substeps"
    if "own waves" in r:
        o = r["own waves"]
        print(f"{head}: lines sharing waves {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) | every line on its own wave {o[0]:.4f} ms "
              f"({o[1]:.4f}..{o[2]:.4f}) = {o[0] / f[0]:.2f} x", flush=True)
    print(f"{head}: ocean_moorings_step (2 launches) {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) | composed route {c[0]:.4f} ms "
          f"({c[1]:.4f}..{c[2]:.4f}) = {c[0] / f[0]:.2f} x | {count * nodes * substeps / (f[0] * 1e-3):.3e} node substeps/s fused | "
          f"largest difference between the routes' nodes after one call {diff:.2e} m", flush=True)
    moorings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x8,1024x64,1x64")
    ap.add_argument("--substeps", default="1,8,64")
    ap.add_argument("--n", type=int, default=256)
    args = ap.parse_args()
    timer = Timer()
    fft = ocean.FFTCalculator(args.n)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.set_depth_layers(DEPTHS)
        g.CalculateOcean(1.0)
        g.calculate_kinematics()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    print(f"{torch.cuda.get_device_name(0)}; 3 x {args.n}^2 cascades, depth layers {DEPTHS}, 4 iterations, tolerance 0; HIP "
          f"events, median (min..max) of 7 alternating windows of 20 calls after 3 warm-ups")
    for shape in args.shapes.split(","):
        count, nodes = (int(v) for v in shape.split("x"))
        for water in (0, 1):
            for substeps in (int(v) for v in args.substeps.split(",")):
                bench_shape(timer, sampler, count, nodes, substeps, water)
    for g in gens:
        g.close()
    fft.close()


if __name__ == "__main__":
    main()
