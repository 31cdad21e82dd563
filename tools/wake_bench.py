#!/usr/bin/env python3
"""Times ocean_wake_step (wake windows).

Windows of M = 256, 1024 and 4096 texels (dx 0.25, sigma 0.5, border 16), a random field loaded, free steps and
steps with 1e4 / 1e6 records, 1 and 8 substeps per call. Record lists in two legs: spread uniformly over the
window, and piled on a 20 x 20 block of texels in random order.

Per shape:
    the call's time for 1 and 8 substeps, and a substep's as (t8 - t1) / 7
    the substep's achieved fraction of its 20 B / texel stream (h read, h_prev read and written, 8 B of the
    accumulator read; 12 B without records) against 8 TB/s, and its flop rate at 340 flop / texel against the
    157 Tflop/s of fp32 vector math, so the log says which of the two binds
    the splat as (t1 with records) - (t1 free) and in records/s, beside foam deposit's yardstick
    (profiles/foam_deposit_bench.log: 1 x 4096^2, 1e6 records, one pair: spread 2.3e9 records/s, pile 9.8e8)

Yardstick: the same step composed from torch ops, conv2d with the 13 x 13 kernel over the zero-padded e, the
elementwise update, and index_put_(accumulate=True) of the float heads for the splat, which is neither bit exact
nor replayable. Both are run from the same state first and compared at 1e-5 of max |h| before timing.

HIP events on the (default) stream all legs share; the median (min..max) of ROUNDS windows of CALLS calls after
WARMUP warm-ups, fewer at 4096. The field decays under the border's damping; the kernels' work does not depend on
the values.

    python tools/wake_bench.py [--sizes 256,1024,4096] [--records 10000,1000000] [--out profiles/wake_bench.log]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DX = 0.25
STEP = dict(gravity=9.8, rho_g=9810.0, damp=0.05, edge_damp=8.0, border=16)
HS = 0.02
HBM = 8.0e12
VALU = 157.3e12


class Log:
    def __init__(self, path):
        self.lines = []
        self.path = path

    def __call__(self, text):
        print(text, flush=True)
        self.lines.append(text)

    def write(self):
        if self.path:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            with open(self.path, "w") as f:
                f.write("\n".join(self.lines) + "\n")


class Composed:
    """The step from torch ops on tensors of its own."""

    def __init__(self, torch, taps, m, h):
        import numpy as np

        self.torch = torch
        idx = np.abs(np.arange(-6, 7))
        self.k = torch.as_tensor(np.ascontiguousarray(taps[np.ix_(idx, idx)]), device="cuda").reshape(1, 1, 13, 13)
        self.m = m
        self.h = h.clone()
        self.hp = torch.zeros_like(h)
        i = torch.arange(m, device="cuda")
        edge = torch.minimum(i, m - 1 - i)
        d = torch.minimum(edge[:, None], edge[None, :]).float()
        border = float(STEP["border"])
        r = torch.clamp(border - d, min=0.0) / border
        self.alpha = STEP["damp"] + STEP["edge_damp"] * r * r

    def step(self, substeps, rec=None):
        torch = self.torch
        m = self.m
        p = torch.zeros(m * m, device="cuda")
        if rec is not None:
            head = rec[:, 5] / (STEP["rho_g"] * DX * DX)
            u, v = rec[:, 0] / DX, rec[:, 2] / DX
            fu, fv = torch.floor(u), torch.floor(v)
            a, b = u - fu, v - fv
            i0, j0 = fu.long(), fv.long()
            for di, dj, w in ((0, 0, (1 - a) * (1 - b)), (1, 0, a * (1 - b)), (0, 1, (1 - a) * b), (1, 1, a * b)):
                i, j = i0 + di, j0 + dj
                ok = (i >= 0) & (i < m) & (j >= 0) & (j < m)
                p.index_put_(((j * m + i)[ok],), (head * w)[ok], accumulate=True)
        p = p.reshape(m, m)
        c = HS * HS * STEP["gravity"] / DX
        b = 0.5 * HS * self.alpha
        for _ in range(substeps):
            e = (self.h + p).reshape(1, 1, m, m)
            acc = torch.nn.functional.conv2d(e, self.k, padding=6).reshape(m, m)
            new = (2.0 * self.h - (1.0 - b) * self.hp - c * acc) / (1.0 + b)
            self.hp, self.h = self.h, new


def lists(torch, count, m):
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda: torch.rand(count, device="cuda", generator=gen)  # noqa: E731
    rec = torch.zeros((count, 8), device="cuda", dtype=torch.float32)
    rec[:, 5] = (rnd() - 0.5) * (2.0e4 / count)  # a few cm of head in all
    spread = rec.clone()
    spread[:, 0], spread[:, 2] = rnd() * (m - 1) * DX, rnd() * (m - 1) * DX
    cell = torch.randint(0, 400, (count,), device="cuda", generator=gen)
    pile = rec.clone()
    pile[:, 0] = ((cell % 20).float() + m // 2 + rnd() * 0.9) * DX
    pile[:, 2] = ((cell // 20).float() + m // 2 + rnd() * 0.9) * DX
    return {"spread": spread, "pile": pile}


def bench_size(log, timer, m, counts):
    import numpy as np
    import torch

    import oceansimulation_amd as ocean
    from mips_bench import _DevicePtr

    fft = ocean.FFTCalculator(64)
    wake = ocean.Wake(fft, m, DX, 0.0, 0.0, 0.5)
    taps = wake.kernel()
    assert HS < wake.max_substep(STEP["gravity"])
    rounds, calls, warmup = (5, 20, 3) if m <= 1024 else (3, 5, 1)
    start = (torch.randn((m, m), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 0.05)
    start = torch.nn.functional.avg_pool2d(start.reshape(1, 1, m, m), 5, stride=1, padding=2).reshape(m, m).contiguous()

    def load():
        wake.reset()
        torch.as_tensor(_DevicePtr(wake.height_ptr(), (m, m)), device="cuda").copy_(start)

    log(f"M = {m} ({m * m * 16 / 2 ** 20:.0f} MiB of state; {rounds} windows of {calls} calls after {warmup}; hs {HS} s):")
    legs = {0: {None: None}}
    for count in counts:
        legs[count] = lists(torch, count, m)
    # the composed step from the same state, before timing
    worst = 0.0
    for count, leg in ((0, None), (counts[0], "spread")):
        rec = legs[count][leg]
        load()
        wake.step_ptr(rec.data_ptr() if rec is not None else 0, count, 0, dt=8 * HS, substeps=8, **STEP)
        fft.synchronize()
        ours = wake.height().clone()
        comp = Composed(torch, taps, m, start)
        comp.step(8, rec)
        torch.cuda.synchronize()
        err = float((ours - comp.h).abs().max()) / float(ours.abs().max())
        worst = max(worst, err)
        log(f"    composed from torch ops, 8 substeps, {count} records: max |a - b| / max |h| = {err:.3e}, within 1e-5: "
            f"{'yes' if err <= 1e-5 else 'NO'}")
    ok = worst <= 1e-5
    free = {}
    for count in [0] + list(counts):
        for leg, rec in legs[count].items():
            t = {}
            for substeps in (1, 8):
                load()

                def call():
                    wake.step_ptr(rec.data_ptr() if rec is not None else 0, count, 0, dt=substeps * HS, substeps=substeps,
                                  **STEP)

                t[substeps] = timer(call, rounds, calls, warmup)
            sub = (t[8][0] - t[1][0]) / 7.0
            per = 20.0 if count else 12.0
            text = (f"    {count:8d} records {leg or 'free':6s}: 1 substep {t[1][0]:.4f} ms ({t[1][1]:.4f}..{t[1][2]:.4f}), "
                    f"8 substeps {t[8][0]:.4f} ms ({t[8][1]:.4f}..{t[8][2]:.4f}); a substep {sub:.4f} ms = "
                    f"{m * m * per / sub / 1e-3 / HBM:.3f} of 8 TB/s at {per:.0f} B/texel, "
                    f"{m * m * 340.0 / sub / 1e-3 / 1e12:.2f} Tflop/s = {m * m * 340.0 / sub / 1e-3 / VALU:.3f} of fp32 vector peak")
            if count == 0:
                free = t
            else:
                splat = t[1][0] - free[1][0]
                text += f"; splat and clear {splat:.4f} ms = {count / max(splat, 1e-6) / 1e-3:.3e} records/s"
            log(text)
    # the yardstick's time: free steps and the first list, spread
    comp = Composed(torch, taps, m, start)
    for count, leg in ((0, None), (counts[0], "spread"), (counts[-1], "spread")):
        rec = legs[count][leg]
        tc1 = timer(lambda: comp.step(1, rec), rounds, calls, warmup)
        tc8 = timer(lambda: comp.step(8, rec), rounds, max(calls // 4, 2), warmup)
        log(f"    torch ops, {count} records: 1 substep {tc1[0]:.4f} ms, 8 substeps {tc8[0]:.4f} ms ({tc8[1]:.4f}..{tc8[2]:.4f})")
    wake.close()
    fft.close()
    del legs
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--records", default="10000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wake_bench.log"))
    args = ap.parse_args()
    import torch  # first: one HIP runtime per process (tests/conftest.py)

    from foam_deposit_bench import Timer

    log = Log(args.out)
    log("HIP events, median (min..max) per call; dx 0.25, sigma 0.5, border 16, damp 0.05, edge_damp 8")
    ok = True
    for m in [int(v) for v in args.sizes.split(",")]:
        ok = bench_size(log, Timer(torch), m, [int(v) for v in args.records.split(",")]) and ok
    log("library and torch composition within 1e-5 of max |h| at every size: " + ("yes" if ok else "NO"))
    log.write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
