#!/usr/bin/env python3
"""Times ocean_particles_step (spray particles).

Pools of about 1e4, 1e6 and 1.6e7 live particles on 3 x 256^2 (the reference scene, one batched generator) and
1 x 4096^2, every shape after eight frames of CalculateOcean(0.25) with rates calculated. The timed list is in a
steady state: particles at rest 50 m above the water, no gravity, no drag, lifetime +inf, so every step moves,
queries and keeps every particle and the next step sees the same list. That is stage 3's worst case (32 B read and
32 B written for every particle); a list that lands or expires particles shrinks from call to call.

Default mode: the step against the same step composed from torch ops on the list (the integration and the fates),
ocean_surface_query on the moved positions, boolean-mask compaction (which synchronises the host to learn the
counts), torch.cat for the append after reading the emitter's count on the host; both legs in one process,
alternating round by round. Before timing, both routes step a list with all three fates and an emission
(threshold 1.0, rate 64) into a pool that the append fills, and the lists, the impacts and the counts are compared
bit for bit; the tool exits non-zero if they differ. HIP events on the (default) stream all legs share, CALLS calls
after WARMUP warm-ups per window, the median of ROUNDS windows per leg.

--kernels: the three kernels' times. One child process per shape and pool under `rocprofv3 --kernel-trace` (a run
of its own: tracing slows the host), 40 steps after 5 warm-ups; per kernel the median duration, and stage 3's
share of 8 TB/s at its 64 B per particle.

    python tools/particles_bench.py [--shapes 3x256,1x4096] [--pools 10000,1000000,16000000] [--kernels]
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

DT, SEED, STEP = 0.25, 12345, 7
PEAK = 8e12  # B/s
KERNELS = ("k_particles_move", "k_particles_scan", "k_particles_scatter")
REST = dict(gravity=0.0, drag=0.0, lifetime=float("inf"))  # the steady list
MIXED = dict(lifetime=1.0)                                 # the compared list


def scene(cascades, n):
    from spray_bench import scene as spray_scene

    return spray_scene(cascades, n)


def extent(g, cascades):
    return max(g.GetOceanSettings(c).planeSize for c in range(cascades))


def resting(torch, alive, size):
    """`alive` particles at rest 50 m above the water, spread over size x size metres."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    rec = torch.zeros((alive, 8), device="cuda", dtype=torch.float32)
    rec[:, 0] = torch.rand(alive, device="cuda", generator=gen) * size
    rec[:, 2] = torch.rand(alive, device="cuda", generator=gen) * size
    rec[:, 1] = 50.0
    rec.view(torch.int32)[:, 7] = torch.arange(alive, device="cuda", dtype=torch.int32)
    return rec


def mixed(torch, alive, size):
    """Heights within a few metres of the water, ages over twice MIXED's lifetime: all three fates."""
    gen = torch.Generator(device="cuda").manual_seed(2)
    rec = resting(torch, alive, size)
    rec[:, 1] = torch.rand(alive, device="cuda", generator=gen) * 4.0 - 1.0
    rec[:, 3] = torch.rand(alive, device="cuda", generator=gen) * 2.0
    rec[:, 4:7] = torch.rand((alive, 3), device="cuda", generator=gen) * 4.0 - 2.0
    return rec


def composed_step(torch, sampler, rec, s, dt, emitter=None, emit=None, capacity=None):
    """The step from torch ops and ocean_surface_query: (next list, impacts, counts as a list)."""
    alive = rec.shape[0]
    wind = torch.tensor(list(s.wind), device="cuda", dtype=torch.float32)
    u = rec[:, 4:7]
    a = (wind - u) * s.drag
    a[:, 1] -= s.gravity
    u2 = u + a * dt
    p2 = rec[:, 0:3] + u2 * dt
    age = rec[:, 3] + dt
    xz = p2[:, [0, 2]].contiguous()
    q = torch.empty((max(alive, 1), 8), device="cuda", dtype=torch.float32)
    sampler.query(xz.data_ptr(), alive, s.iterations, s.tolerance, q.data_ptr())
    w = q[:alive, 1]
    landed = ~(p2[:, 1] > w)
    expired = ~landed & ~(age < s.lifetime)
    moved = torch.cat([p2, age[:, None], u2, rec[:, 7:8]], 1)
    nxt = moved[~(landed | expired)]  # synchronises: the count reaches the host
    hit = moved[landed]
    hit[:, 1] = w[landed]
    survivors, appended, emitted = nxt.shape[0], 0, 0
    if emit is not None:
        emitted = int(emitter.counts()[0])  # synchronises
        appended = min(emitted, capacity - survivors)
        e = emit[:appended]
        new = torch.cat([e[:, 0:3], torch.zeros_like(e[:, 3:4]), e[:, 4:5] * s.gain,
                         (e[:, 5] * s.gain + e[:, 3] * s.lift)[:, None], e[:, 6:7] * s.gain, e[:, 7:8]], 1)
        nxt = torch.cat([nxt, new])
    counts = [survivors + appended, alive, survivors, hit.shape[0], hit.shape[0], int(expired.sum()), appended,
              emitted - appended]
    return nxt, hit, counts


def compare(torch, np, fft, g, sampler, emitter, cascades, n, alive):
    """One step of a list with all three fates and an emission that fills the pool, both routes: identical?"""
    import oceansimulation_amd as ocean
    from mips_bench import _DevicePtr
    from oceansimulation_amd.surface import SprayParticles

    s = ocean.default_particle_settings(**MIXED)
    emit = torch.empty((cascades * n * n, 8), device="cuda", dtype=torch.float32)
    emitter.emit(sampler, dict(threshold=1.0, rate=64.0, seed=SEED), DT, STEP, emit.data_ptr(), emit.shape[0])
    rec = mixed(torch, alive, extent(g, cascades))
    capacity = alive + 16
    pool = SprayParticles(fft, capacity)
    pool.load(rec.data_ptr(), alive)
    hit = torch.full((alive, 8), float("nan"), device="cuda", dtype=torch.float32)
    pool.step(sampler, s, DT, emitter=emitter, emit_records=emit.data_ptr(), landed=hit.data_ptr(), landed_capacity=alive)
    counts = pool.counts().tolist()
    got = torch.as_tensor(_DevicePtr(pool.records_ptr, (max(counts[0], 1), 8)), device="cuda")[:counts[0]]
    nxt, want_hit, want_counts = composed_step(torch, sampler, rec, s, DT, emitter, emit, capacity)
    bits = lambda t: t.contiguous().cpu().numpy().view(np.uint32)  # noqa: E731
    same = (counts == want_counts and np.array_equal(bits(got), bits(nxt)) and
            np.array_equal(bits(hit[:counts[4]]), bits(want_hit)))
    pool.close()
    return same, counts


def bench_shape(timer, cascades, n, pools):
    import numpy as np
    import torch

    import oceansimulation_amd as ocean
    from oceansimulation_amd.surface import SprayParticles

    fft, g, sampler, emitter = scene(cascades, n)
    ok = True
    s = ocean.default_particle_settings(**REST)
    for alive in pools:
        same, counts = compare(torch, np, fft, g, sampler, emitter, cascades, n, min(alive, 1000000))
        ok = ok and same
        rec = resting(torch, alive, extent(g, cascades))
        pool = SprayParticles(fft, alive)
        pool.load(rec.data_ptr(), alive)

        def fused():
            pool.step(sampler, s, DT)

        def composed():
            return composed_step(torch, sampler, rec, s, DT)

        fused()
        assert pool.counts().tolist() == [alive, alive, alive, 0, 0, 0, 0, 0]
        res = timer.alternating({"fused": fused, "composed": composed})
        torch.cuda.synchronize()
        assert pool.counts().tolist() == [alive, alive, alive, 0, 0, 0, 0, 0]
        f, c = res["fused"], res["composed"]
        print(f"{cascades} x {n}^2, {alive} particles: ocean_particles_step {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}; "
              f"3 launches, no host synchronisation) | composed from torch ops, ocean_surface_query, mask compaction "
              f"{c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f}) = {c[0] / f[0]:.2f} x | mixed list of {counts[1]} "
              f"(survivors {counts[2]}, landed {counts[3]}, expired {counts[5]}, appended {counts[6]}, dropped "
              f"{counts[7]}) identical: {'yes' if same else 'NO'}", flush=True)
        pool.close()
        del rec
        torch.cuda.empty_cache()
    emitter.close()
    g.close()
    fft.close()
    return ok


def run_timing(shapes, pools):
    import torch  # noqa: F401  first: one HIP runtime per process (tests/conftest.py)

    from mips_bench import Timer

    timer = Timer()
    print("HIP events, median (min..max) of 5 alternating windows of 20 calls after 3 warm-ups", flush=True)
    ok = True
    for cascades, n in shapes:
        ok = bench_shape(timer, cascades, n, pools) and ok
    print("lists, impacts and counts identical to the composed step at every shape and pool: " + ("yes" if ok else "NO"),
          flush=True)
    return 0 if ok else 1


def run_child(cascades, n, alive):
    """The calls one profiler run traces: 5 warm-ups and 40 steps of the steady list."""
    import torch

    import oceansimulation_amd as ocean
    from oceansimulation_amd.surface import SprayParticles

    fft, g, sampler, emitter = scene(cascades, n)
    rec = resting(torch, alive, extent(g, cascades))
    pool = SprayParticles(fft, alive)
    pool.load(rec.data_ptr(), alive)
    s = ocean.default_particle_settings(**REST)
    for _ in range(45):
        pool.step(sampler, s, DT)
    print(f"alive {int(pool.counts()[0])}", flush=True)
    return 0


def run_kernels(shapes, pools):
    print("rocprofv3 --kernel-trace, one process per shape and pool: median kernel time of the last 40 of 45 steps",
          flush=True)
    for cascades, n in shapes:
        for alive in pools:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "particles", "--",
                       sys.executable, os.path.abspath(__file__), "--child", f"{cascades}x{n}", str(alive)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    return r.returncode
                times = {k: [] for k in KERNELS}
                for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    with open(f) as fh:
                        for row in csv.DictReader(fh):
                            for k in KERNELS:
                                if k in row["Kernel_Name"]:
                                    times[k].append((int(row["Start_Timestamp"]),
                                                     (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
            med = {k: statistics.median(t for _, t in sorted(v)[-40:]) if v else float("nan") for k, v in times.items()}
            frac = alive * 64 / (med["k_particles_scatter"] * 1e-6) / PEAK
            print(f"{cascades} x {n}^2, {alive} particles: " + ", ".join(f"{k} {med[k]:.2f} us" for k in KERNELS) +
                  f" | stage 3: {frac:.3f} of 8 TB/s at 64 B per particle", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x256,1x4096")
    ap.add_argument("--pools", default="10000,1000000,16000000")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "ALIVE"))
    args = ap.parse_args()
    if args.child:
        c, n = args.child[0].split("x")
        return run_child(int(c), int(n), int(args.child[1]))
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    pools = [int(v) for v in args.pools.split(",")]
    return run_kernels(shapes, pools) if args.kernels else run_timing(shapes, pools)


if __name__ == "__main__":
    sys.exit(main())
