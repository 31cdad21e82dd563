#!/usr/bin/env python3
"""Times ocean_camera_render (camera images) and writes profiles/camera_bench.log.

3 x 256^2 cascades (the reference scene, three generators), ocean_default_camera (far 1500), the default
shading and march, at 640 x 480 and 1025 x 1025. Three legs in the same process, alternating round by round:
  (a) fused     ocean_camera_render writing image, aux and image8 (and once more the image alone)
  (b) composed  the same picture on the calls the library had before: ocean_surface_raycast on the same rays
                (made once by ocean_camera_rays, not timed), ocean_surface_sample at the hits' base points for
                V, then the header's shading as torch elementwise fp32 operations in the contract's order
  (c) march     ocean_surface_raycast alone on the same rays
Before timing, (a) and (b) are compared per channel against the gate of tests/test_camera.py,
|a - b| <= 2^-20 * (|col| + |sky(d)|); a miss ends the run with status 1.
HIP events on the (default) stream all legs share, CALLS calls after WARMUP warm-ups per window, the median
of ROUNDS windows per leg. The two ratios: a / c (what the shading and the tile mapping cost or save over the
bare march) and b / a.

    python tools/camera_bench.py [--sizes 640x480,1025x1025] [--log profiles/camera_bench.log]
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

import camera_ref as CR  # noqa: E402
import oceansimulation_amd as ocean  # noqa: E402
from mips_bench import PLANES, Timer, _DevicePtr  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer  # noqa: E402
from oceansimulation_amd.surface import (SurfaceSampler, camera_rays_host, default_camera, default_march,  # noqa: E402
                                         default_shading)

GATE = 2.0 ** -20


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(v):
    return v / torch.sqrt(_dot(v, v))[:, None]


class TorchShading:
    """The header's sky / water / fog as torch fp32 elementwise operations, one kernel per operation."""

    def __init__(self, cam, shading):
        L, cthr, cfade = CR.host_constants(shading)
        dev = "cuda"
        self.L = torch.tensor(L, device=dev)[None, :]
        self.cthr, self.cfade = float(cthr), float(cfade)
        self.sky_c = torch.tensor(list(shading.sky_color), device=dev)[None, :]
        self.light_c = torch.tensor(list(shading.light_color), device=dev)[None, :]
        self.wave_c = torch.tensor(list(shading.wave_color), device=dev)[None, :]
        self.scatter_c = torch.tensor(list(shading.scatter_color), device=dev)[None, :]
        self.pos = torch.tensor(list(cam.position), device=dev)[None, :]
        self.fog_begin, self.fog_density = float(shading.fog_begin), float(shading.fog_density)

    def sky(self, v):
        u = _normalize(v)
        s = _dot(self.L, u)
        e = torch.clamp((s - self.cfade) / (self.cthr - self.cfade), 0.0, 1.0)
        w = (e * e) * (3.0 - 2.0 * e)
        w = w * (w * w)
        m = 0.8 - u[:, 1] / 0.8
        m = m * m
        box = self.sky_c * (1.0 - m)[:, None] + self.light_c * m[:, None]
        return (1.0 - w)[:, None] * box + (2.0 * w)[:, None] * self.light_c

    def __call__(self, hits, V, d, length):
        """hits (n, 16) raycast rows, V (n, 8) ocean_surface_sample at the base points -> image (n, 4), col, sky_d."""
        P, n = V[:, 0:3], hits[:, 4:7]
        z = hits[:, 3] / length
        sky_d = self.sky(d)
        I = -_normalize(self.pos - P)
        k = 2.0 * _dot(n, I)
        r = I - k[:, None] * n
        diffuse = torch.clamp_min(_dot(n, self.L), 0.0) * 0.3
        sp = torch.clamp_min(_dot(r, self.L), 0.0)
        for _ in range(5):
            sp = sp * sp
        light = (diffuse + 0.5) + sp * 0.5
        scatter = torch.clamp_min(P[:, 1] * 0.1, 0.0)
        col = ((light[:, None] * self.wave_c) * self.sky(r)) + scatter[:, None] * self.scatter_c
        f = torch.clamp_min(1.0 - torch.exp(-((z - self.fog_begin) * self.fog_density)), 0.0)
        out = col * (1.0 - f)[:, None] + sky_d * f[:, None]
        hit = (hits[:, 12] == 0)[:, None]
        out = torch.where(hit, out, sky_d)
        image = torch.cat([out, torch.ones_like(out[:, :1])], 1)
        return image, torch.where(hit, col, torch.zeros_like(col)), sky_d


def bench(timer, sampler, w, h, say):
    cam, sh, march = default_camera(), default_shading(), default_march()
    n = w * h
    rays_host = camera_rays_host(cam, w, h)
    _, length_host = CR.camera_rays(cam, w, h)
    rays = DeviceBuffer.from_array(rays_host)
    hits_buf = DeviceBuffer(n * 64)
    image, aux, image8 = DeviceBuffer(n * 16), DeviceBuffer(n * 16), DeviceBuffer(n * 4)
    r = torch.as_tensor(_DevicePtr(rays.ptr, (n, 8)), device="cuda")
    hits = torch.as_tensor(_DevicePtr(hits_buf.ptr, (n, 16)), device="cuda")
    length = torch.tensor(length_host, device="cuda")
    base = torch.empty((n, 2), device="cuda")
    V = torch.empty((n, 8), device="cuda")
    shade = TorchShading(cam, sh)
    kw = dict(step=march.step, max_steps=march.max_steps, refine=march.refine, iterations=march.iterations,
              tolerance=march.tolerance, slope=march.slope, pad=march.pad)

    def fused():
        sampler.render(cam, sh, march, w, h, image.ptr, aux.ptr, image8.ptr)

    def fused_image():
        sampler.render(cam, sh, march, w, h, image.ptr, 0, 0)

    def cast():
        sampler.raycast(rays.ptr, n, hits_buf.ptr, **kw)

    def composed():
        cast()
        torch.stack((hits[:, 8], hits[:, 10]), 1, out=base)
        sampler.sample(base.data_ptr(), n, V.data_ptr())
        return shade(hits, V, r[:, 4:7], length)

    fused()
    b_image, b_col, b_sky = composed()
    torch.cuda.synchronize()
    a_image = torch.as_tensor(_DevicePtr(image.ptr, (n, 4)), device="cuda")
    diff = (a_image[:, :3].double() - b_image[:, :3].double()).abs()
    bound = GATE * (b_col.abs() + b_sky.abs()).double()
    ok = bool((diff <= bound).all())
    worst = float((diff / bound).max())
    a_aux = aux.to_host((n, 4))
    hit = int((a_aux[:, 3] == 0).sum())
    say(f"{w} x {h} ({n} pixels, {hit} hit the water, mean marching steps per ray "
        f"{float(hits[:, 14].mean()):.1f}): fused and composed pictures agree within the gate: "
        f"{'yes' if ok else 'NO'} (worst |a - b| / bound {worst:.3f}, {int((diff > 0).sum())} of {3 * n} channels differ)")
    if not ok:
        return False
    res = timer.alternating({"a": fused, "a_image": fused_image, "b": composed, "c": cast})
    torch.cuda.synchronize()
    a, ai, b, c = res["a"], res["a_image"], res["b"], res["c"]
    say(f"    (a) ocean_camera_render, image + aux + image8 {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}) = "
        f"{n / (a[0] * 1e-3):.3e} pixels/s; image alone {ai[0]:.4f} ms ({ai[1]:.4f}..{ai[2]:.4f})")
    say(f"    (b) raycast + sample + torch shading {b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f})")
    say(f"    (c) ocean_surface_raycast alone {c[0]:.4f} ms ({c[1]:.4f}..{c[2]:.4f})")
    say(f"    a / c = {a[0] / c[0]:.3f}, b / a = {b[0] / a[0]:.2f}; (a) slower than (b): {'YES' if a[0] > b[0] else 'no'}")
    for buf in (rays, hits_buf, image, aux, image8):
        buf.free()
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1025x1025")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "camera_bench.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    timer = Timer()
    say("HIP events, median (min..max) of 5 alternating windows of 20 calls after 3 warm-ups; 3 x 256^2 cascades, "
        "ocean_default_camera / _shading / _march")
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.BuildBounds()
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    ok = True
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        ok = bench(timer, sampler, w, h, say) and ok
    fft.synchronize()
    for g in gens:
        g.close()
    fft.close()
    log.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
