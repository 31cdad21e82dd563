#!/usr/bin/env python3
"""Times ocean_spray_emit (spray emitters).

Threshold 0.9 with rates 8 and 1e30, dt 1/60, on 3 x 256^2 (the reference scene, one batched generator),
1 x 4096^2 and 8 x 4096^2 (the first 8 cascades of one generator), every shape after eight frames of
CalculateOcean(0.25) with rates calculated.

Default mode: the whole call with room for exactly `found` records against the same list composed from torch
ops on the exposed Jacobian maps (the predicate with the counter hash restated on int64 tensors, the hash of
(x, y) precomputed), torch.nonzero (which synchronises the host to learn the count), gathers and
ocean_surface_velocity on the base points, both legs in one process, alternating round by round; also the
counting-only call. Before timing, both routes' records are compared bit for bit; the tool exits non-zero if
they differ. HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window,
the median of ROUNDS windows per leg.

--kernels: the four kernels' times. One child process per shape and rate under
`rocprofv3 --kernel-trace` (a run of its own: tracing slows the host), 40 calls after 5 warm-ups; per kernel the
median duration, and stage 1's share of 8 TB/s at its 4 B per texel.

    python tools/spray_bench.py [--shapes 3x256,1x4096,8x4096] [--kernels]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

THRESHOLD, RATES, DT, SEED, STEP = 0.9, (8.0, 1e30), 1.0 / 60.0, 12345, 7
PEAK = 8e12  # B/s
PLANES = (5.0, 17.0, 101.0)
KERNELS = ("k_spray_count", "k_spray_scan", "k_spray_scatter", "k_spray_fill")


def scene(cascades, n):
    """(fft, generator, sampler over its cascades, emitter) after eight frames, rates calculated."""
    import oceansimulation_amd as ocean
    from oceansimulation_amd.surface import SprayEmitter, SurfaceSampler

    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3] * (1 + c // 3), seed=(c, 2 * c))
    for k in range(8):
        g.CalculateOcean(0.25, k == 0)
    g.calculate_rates()
    fft.synchronize()
    return fft, g, SurfaceSampler([(g, c) for c in range(cascades)]), SprayEmitter(fft)


def settings(rate):
    return dict(threshold=THRESHOLD, rate=rate, seed=SEED)


def _hash_raw(x, y):
    """device/spectrum.h's hash_raw on int64 tensors holding uint32 values"""
    m = 0xFFFFFFFF
    h = (y + 374761393 + x * 3266489917) & m
    h = (2246822519 * (h ^ (h >> 15))) & m
    h = (3266489917 * (h ^ (h >> 13))) & m
    return h ^ (h >> 16)


def bench_shape(timer, cascades, n):
    import numpy as np
    import torch

    from mips_bench import _DevicePtr

    fft, g, sampler, emitter = scene(cascades, n)
    nn = n * n
    jac = torch.as_tensor(_DevicePtr(g.GetJacobianMap(0), (cascades, nn)), device="cuda")
    texel = torch.arange(nn, device="cuda", dtype=torch.int64)
    hxy = _hash_raw(texel % n, texel // n)  # the same for every step: kept by a user too
    plane = torch.tensor([g.GetOceanSettings(c).planeSize for c in range(cascades)], device="cuda", dtype=torch.float32)
    cell = plane / np.float32(n)
    ok = True
    for rate in RATES:
        emitter.emit(sampler, settings(rate), DT, STEP)
        found = int(emitter.counts()[1])
        out = torch.empty((max(found, 1), 8), device="cuda", dtype=torch.float32)

        def fused():
            emitter.emit(sampler, settings(rate), DT, STEP, out.data_ptr(), found)

        def count_only():
            emitter.emit(sampler, settings(rate), DT, STEP)

        def composed():
            d = THRESHOLD - jac
            p = torch.clamp_min(d, 0.0).mul_(rate).mul_(DT).clamp_max_(1.0)
            nh = _hash_raw(hxy ^ SEED, STEP)
            u = ((nh >> 1) & 0x7FFFFFFF).to(torch.float32) / 2147483648.0
            emits = (d > 0) & ((p >= 1.0) | (u < p))
            idx = torch.nonzero(emits.view(-1)).view(-1)  # synchronises: the count reaches the host
            pair, t = idx // nn, idx % nn
            xz = torch.stack([((t % n).to(torch.float32) + 0.5) * cell[pair],
                              ((t // n).to(torch.float32) + 0.5) * cell[pair]], 1).contiguous()
            rec = torch.empty((max(idx.numel(), 1), 8), device="cuda", dtype=torch.float32)
            if idx.numel():
                sampler.velocity(xz.data_ptr(), idx.numel(), rec.data_ptr())
                rec[:idx.numel(), 3] = d.view(-1)[idx]
                rec.view(torch.int32)[:idx.numel(), 7] = ((pair << 28) | t).to(torch.int32)
            return rec, idx.numel()

        fused()
        fft.synchronize()
        rec, count = composed()
        torch.cuda.synchronize()
        same = count == found and np.array_equal(out[:found].cpu().numpy().view(np.uint32),
                                                 rec[:found].cpu().numpy().view(np.uint32))
        ok = ok and same
        res = timer.alternating({"fused": fused, "count": count_only, "composed": composed})
        torch.cuda.synchronize()
        f, k, c = res["fused"], res["count"], res["composed"]
        print(f"{cascades} x {n}^2, rate {rate:g}: found {found} of {cascades * nn} ({found / (cascades * nn):.4f}) | "
              f"ocean_spray_emit {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}; 4 launches, no host synchronisation) | "
              f"counting only {k[0]:.4f} ms ({k[1]:.4f}..{k[2]:.4f}; 2 launches) | composed from torch.nonzero, "
              f"gathers and ocean_surface_velocity {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}) = {c[0] / f[0]:.2f} x | "
              f"records identical: {'yes' if same else 'NO'}", flush=True)
        del out, rec
    del jac, texel, hxy
    torch.cuda.empty_cache()
    emitter.close()
    g.close()
    fft.close()
    return ok


def run_timing(shapes):
    import torch  # noqa: F401  first: one HIP runtime per process (tests/conftest.py)

    from mips_bench import Timer

    timer = Timer()
    print("HIP events, median (min..max) of 5 alternating windows of 20 calls after 3 warm-ups", flush=True)
    ok = True
    for cascades, n in shapes:
        ok = bench_shape(timer, cascades, n) and ok
    print("records identical to the composed list at every shape and rate: " + ("yes" if ok else "NO"), flush=True)
    return 0 if ok else 1


def run_child(cascades, n, rate):
    """The calls one profiler run traces: 5 warm-ups and 40 calls with room for exactly `found` records."""
    import torch  # noqa: F401

    from oceansimulation_amd.hip import DeviceBuffer

    fft, g, sampler, emitter = scene(cascades, n)
    emitter.emit(sampler, settings(rate), DT, STEP)
    found = int(emitter.counts()[1])
    out = DeviceBuffer(max(found, 1) * 32)
    for _ in range(45):
        emitter.emit(sampler, settings(rate), DT, STEP, out.ptr, found)
    fft.synchronize()
    print(f"found {found}", flush=True)
    return 0


def run_kernels(shapes):
    print("rocprofv3 --kernel-trace, one process per shape and rate: median kernel time of the last 40 of 45 calls",
          flush=True)
    for cascades, n in shapes:
        for rate in RATES:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "spray", "--",
                       sys.executable, os.path.abspath(__file__), "--child", f"{cascades}x{n}", str(rate)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    return r.returncode
                found = [line for line in r.stdout.splitlines() if line.startswith("found ")]
                times = {k: [] for k in KERNELS}
                for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    with open(f) as fh:
                        for row in csv.DictReader(fh):
                            for k in KERNELS:
                                if k in row["Kernel_Name"]:
                                    times[k].append((int(row["Start_Timestamp"]),
                                                     (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
            med = {k: statistics.median(t for _, t in sorted(v)[-40:]) if v else float("nan") for k, v in times.items()}
            points = cascades * n * n
            frac = points * 4 / (med["k_spray_count"] * 1e-6) / PEAK
            print(f"{cascades} x {n}^2, rate {rate:g} ({found[0] if found else 'found ?'}): " +
                  ", ".join(f"{k} {med[k]:.2f} us" for k in KERNELS) +
                  f" | stage 1: {frac:.3f} of 8 TB/s at 4 B per texel", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096,8x4096")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "RATE"))
    args = ap.parse_args()
    if args.child:
        c, n = args.child[0].split("x")
        return run_child(int(c), int(n), float(args.child[1]))
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    return run_kernels(shapes) if args.kernels else run_timing(shapes)


if __name__ == "__main__":
    sys.exit(main())
