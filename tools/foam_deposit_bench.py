#!/usr/bin/env python3
"""Times ocean_foam_deposit (foam deposit).

Scenes: 3 x 256^2 (the reference scene, one batched generator) and 1 x 4096^2, eight frames of CalculateOcean(0.25)
each followed by a foam step. Record lists of 1e4, 1e6 and 1.6e7 records, uy in -10 .. 2 m/s, settings
(amount, per_speed) = (0.002, 0.0005) on every pair, in three legs:

    spread   uniform over the largest plane
    pile     on about 400 texels of the coarsest cascade (a 20 x 20 block of them), in random order
    sorted   the same pile sorted by texel, as an ordered impact list seen by a coarse cascade is

each with and without the merge within the wave (ocean_debug_foam_deposit_merge): the counts of both variants must
be equal. Per leg: the time of a call (three launches), records/s and accumulator adds/s (the taps with units, what
the unmerged variant issues), to set beside the camera splat's 1.3e10 min + add pairs/s
(profiles/camera_layers_bench.log). Traffic per record: 12 B of its 32-B record read in each of the two passes
(64 B of whole lines for a dense list), and per active pair 4 adds of 8 B, 4 filter loads of 8 B and, per texel it
is the first to reach, an 8-B exchange and 4 B of foam read and written.

Yardstick: the same deposit composed from torch ops (the taps in float32, index_put_(accumulate=True) of
d * w on the foam maps through their device pointers, clamp), timed on the spread leg and compared with the
library's maps within 1e-5 only: a float scatter is neither ordered nor quantised to 2^-24.

HIP events on the (default) stream all legs share; the median (min..max) of ROUNDS windows of CALLS calls after
WARMUP warm-ups, fewer for the long lists. Foam saturates under repeated deposits; the kernels' work does not depend
on the foam's values.

    python tools/foam_deposit_bench.py [--shapes 3x256,1x4096] [--records 10000,1000000,16000000]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PLANES = (5.0, 17.0, 101.0)
SETTINGS = dict(amount=0.002, per_speed=0.0005)
FOAM = dict(bias=1.0, gain=32.0, decay=0.5, level=0.5)


def scene(cascades, n):
    import oceansimulation_amd as ocean
    from oceansimulation_amd.surface import SurfaceSampler

    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[(c + 3 - cascades) % 3])
        ocean.apply_foam_settings(g.GetFoamSettings(c), **FOAM)
    for k in range(8):
        g.CalculateOcean(0.25, k == 0)
        g.AdvanceFoam(0.25)
    fft.synchronize()
    return fft, g, SurfaceSampler([(g, c) for c in range(cascades)])


def lists(torch, count, n, plane):
    """{leg: (count, 8) float32 device records}"""
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda: torch.rand(count, device="cuda", generator=gen)  # noqa: E731
    rec = torch.zeros((count, 8), device="cuda", dtype=torch.float32)
    rec[:, 5] = rnd() * 12.0 - 10.0
    spread = rec.clone()
    spread[:, 0], spread[:, 2] = rnd() * plane, rnd() * plane
    texel = plane / n
    cell = torch.randint(0, 400, (count,), device="cuda", generator=gen)
    pile = rec.clone()
    pile[:, 0] = ((cell % 20).float() + 3.0 + rnd() * 0.9) * texel
    pile[:, 2] = ((cell // 20).float() + 3.0 + rnd() * 0.9) * texel
    order = torch.argsort(cell, stable=True)
    return {"spread": spread, "pile": pile, "sorted": pile[order].contiguous()}


class Timer:
    def __init__(self, torch):
        self.torch = torch

    def __call__(self, call, rounds, calls, warmup):
        torch = self.torch
        t = []
        for _ in range(rounds):
            for _ in range(warmup):
                call()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) / calls)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]


def composed(torch, foams, planes, n, rec, s):
    """The deposit from torch ops, in place on the foam maps (flat float32 views)."""
    px, pz = rec[:, 0], rec[:, 2]
    d = s["amount"] + s["per_speed"] * torch.clamp(-rec[:, 5], min=0.0)
    for fm, plane in zip(foams, planes):
        u, v = px / plane * n - 0.5, pz / plane * n - 0.5
        fu, fv = torch.floor(u), torch.floor(v)
        a, b = u - fu, v - fv
        i0, j0 = fu.long() % n, fv.long() % n
        i1, j1 = (i0 + 1) % n, (j0 + 1) % n
        idx = torch.cat([j0 * n + i0, j0 * n + i1, j1 * n + i0, j1 * n + i1])
        val = torch.cat([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b]) * d.repeat(4)
        fm.index_put_((idx,), val, accumulate=True)
        fm.clamp_(max=1.0)


def bench_shape(timer, cascades, n, counts):
    import numpy as np
    import torch

    from mips_bench import _DevicePtr
    from oceansimulation_amd import capi

    L = capi.lib()
    fft, g, sampler = scene(cascades, n)
    planes = [g.GetOceanSettings(c).planeSize for c in range(cascades)]
    foams = [torch.as_tensor(_DevicePtr(g.GetFoamMap(c), (n * n,)), device="cuda") for c in range(cascades)]
    start = [f.clone() for f in foams]
    ok = True
    for count in counts:
        rounds, calls, warmup = (5, 20, 3) if count <= 100000 else (3, 3, 1)
        legs = lists(torch, count, n, max(planes))
        print(f"{cascades} x {n}^2, {count} records ({rounds} windows of {calls} calls after {warmup}):", flush=True)
        times = {}
        for name, rec in legs.items():
            row = {}
            for merge in (1, 0):
                L.ocean_debug_foam_deposit_merge(merge)

                def call():
                    sampler.deposit_foam(rec.data_ptr(), count, SETTINGS)

                for f, s in zip(foams, start):
                    f.copy_(s)
                call()
                first = sampler.deposit_counts()
                maps = [f.clone() for f in foams]
                row[merge] = (timer(call, rounds, calls, warmup), first, maps)
            L.ocean_debug_foam_deposit_merge(1)
            (tm, cm, mm), (tu, cu, mu) = row[1], row[0]
            same = np.array_equal(cm, cu) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mm, mu))
            ok = ok and same
            taps = int(sum(cm[2 + 3 * c] for c in range(cascades)))
            touched = [int(cm[3 + 3 * c]) for c in range(cascades)]
            times[name] = (tm[0], tu[0])
            print(f"    {name:6s} merged {tm[0]:.4f} ms ({tm[1]:.4f}..{tm[2]:.4f}) = {count / tm[0] / 1e-3:.3e} records/s, "
                  f"{taps / tm[0] / 1e-3:.3e} adds/s | unmerged {tu[0]:.4f} ms ({tu[1]:.4f}..{tu[2]:.4f}) = "
                  f"{taps / tu[0] / 1e-3:.3e} adds/s | unmerged / merged = {tu[0] / tm[0]:.2f} | texels touched {touched}, "
                  f"first call's maps and counts identical: {'yes' if same else 'NO'}", flush=True)
        print(f"    merged: pile / spread (the cost of contention) = {times['pile'][0] / times['spread'][0]:.2f}; "
              f"sorted / spread = {times['sorted'][0] / times['spread'][0]:.2f}", flush=True)
        # the yardstick, on the spread leg
        rec = legs["spread"]
        for f, s in zip(foams, start):
            f.copy_(s)
        sampler.deposit_foam(rec.data_ptr(), count, SETTINGS)
        fft.synchronize()
        ours = [f.clone() for f in foams]
        for f, s in zip(foams, start):
            f.copy_(s)
        composed(torch, foams, planes, n, rec, SETTINGS)
        torch.cuda.synchronize()
        worst = max(float((a - b).abs().max()) for a, b in zip(ours, foams))
        tc = timer(lambda: composed(torch, foams, planes, n, rec, SETTINGS), rounds, calls, warmup)
        print(f"    composed from torch ops (index_put_ accumulate) on the spread leg: {tc[0]:.4f} ms ({tc[1]:.4f}..{tc[2]:.4f}) = "
              f"{tc[0] / times['spread'][0]:.2f} x the merged call; worst |a - b| {worst:.3e}, within 1e-5: "
              f"{'yes' if worst <= 1e-5 else 'no'} (each tap truncates up to 2^-24, {4.0 * count / (n * n):.0f} taps per "
              f"texel of a map)", flush=True)
        del legs, rec
        torch.cuda.empty_cache()
    g.close()
    fft.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096")
    ap.add_argument("--records", default="10000,1000000,16000000")
    args = ap.parse_args()
    import torch  # first: one HIP runtime per process (tests/conftest.py)

    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    counts = [int(v) for v in args.records.split(",")]
    timer = Timer(torch)
    print("HIP events, median (min..max) per call; settings (0.002, 0.0005) on every pair", flush=True)
    ok = True
    for cascades, n in shapes:
        ok = bench_shape(timer, cascades, n, counts) and ok
    print("merged and unmerged identical at every shape, list and leg: " + ("yes" if ok else "NO"), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
