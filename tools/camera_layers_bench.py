#!/usr/bin/env python3
"""Times ocean_camera_render_layers (camera layers) and writes profiles/camera_layers_bench.log.

3 x 256^2 cascades (the reference scene, three generators) after eight foam steps of dt = 0.25,
ocean_default_camera (far 1500), the default shading, march and layers, at 640 x 480 and 1025 x 1025.
  foam     ocean_camera_render_layers with the foam stage (image + aux + aux2 + image8, one launch) against
           ocean_camera_render on the same camera (image + aux + image8): the existing call in the same build
  spray    the layered call with foam off and a record list of 1e4, 1e6 and 1.6e7 records against the same call
           with one record: the difference is what the splat costs for the list (the water pass and the
           composite run in both). Two lists: "spread", a record per random pixel, and "dense", every record
           inside one block of 16 x 16 pixels (20 x 20 with the sprites' margins); all at depths 2 .. 8 m, in
           front of the water, where the default sprite is 5 x 5 pixels: 25 min / add pairs per record. The ratio
           dense / spread is the cost of contention. A third list, "sorted", is the dense one ordered by pixel, as
           an ordered list arrives from far away: neighbouring lanes then share pixels and merge before the
           atomics.
  composed the same picture on the calls the library had before: tools/camera_bench.py's composed leg
           (ocean_surface_raycast, the sample at the base points, torch shading) with ocean_surface_sample_foam
           for the sample and the foam mix in torch, then the spray as torch scatter ops (scatter_reduce amin on
           int64 keys, scatter_add on counts, over records x 25 expanded sprite pixels) and the composite in
           torch. Compared with the layered call before timing: aux2's foam, counts and indices must be equal,
           the picture within the three terms of tests/test_camera_layers.py's gate taken on every pixel (torch
           writes some of the shading in another order); a miss ends the run with status 1. Run for 1e4 and
           1e6 records; at 1.6e7 the expanded arrays alone are 400 M entries of 8 + 8 + 4 bytes and the leg is
           left out.
Not expressible on the older calls: the foam under the fog on ocean_camera_render's own output (the fog is
mixed inside the fused kernel, and its aux has no base point to sample the foam at), which is why the composed
leg starts from the ray cast instead.
HIP events on the (default) stream all legs share; the picture legs CALLS calls after WARMUP warm-ups per
window and the median of ROUNDS alternating windows, the record legs 1 warm-up and 3 calls per window.

    python tools/camera_layers_bench.py [--sizes 640x480,1025x1025] [--records 10000,1000000,16000000]
                                        [--log profiles/camera_layers_bench.log]
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
import mips_bench  # noqa: E402
import oceansimulation_amd as ocean  # noqa: E402
from camera_bench import TorchShading, _dot  # noqa: E402
from mips_bench import PLANES, Timer, _DevicePtr  # noqa: E402
from oceansimulation_amd.hip import DeviceBuffer  # noqa: E402
from oceansimulation_amd.surface import (SurfaceSampler, camera_layers_scratch_bytes, camera_rays_host,  # noqa: E402
                                         default_camera, default_camera_layers, default_march, default_shading)

GATE = 2.0 ** -20
FOAM_DT, FOAM_STEPS = 0.25, 8


def points_on_pixels(cam, w, h, i, j, depth):
    """World points (n, 3) at view depth `depth` on the rays of the pixels (i, j): torch float32 on the device."""
    T = float(np.float32(cam.tan_half_fov_y))
    x = ((2.0 * (i + 0.5)) / w - 1.0) * ((w / h) * T)
    y = (1.0 - (2.0 * (j + 0.5)) / h) * T
    vec = lambda a: torch.tensor(list(a), device="cuda", dtype=torch.float32)[None, :]
    d = x[:, None] * vec(cam.right) + y[:, None] * vec(cam.up) + vec(cam.forward)
    return vec(cam.position) + depth[:, None] * d


def record_list(cam, w, h, n, dense, seed, ordered=False):
    """(n, 8) float32 records on the device: spread over the picture, or inside one 16 x 16 pixel block; ordered:
    sorted by pixel, as an ordered list (an emitter's, by texel) arrives from far away."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    u = torch.rand((3, n), device="cuda", generator=g)
    if dense:
        i, j = w // 2 + 16.0 * u[0], h // 3 + 16.0 * u[1]
    else:
        i, j = w * u[0], h * u[1]
    if ordered:
        order = torch.argsort(torch.floor(j) * w + torch.floor(i))
        i, j = i[order], j[order]
    rec = torch.zeros((n, 8), device="cuda")
    rec[:, :3] = points_on_pixels(cam, w, h, i - 0.5, j - 0.5, 2.0 + 6.0 * u[2])
    return rec


class TorchLayers:
    """The layers' part of the contract as torch operations on top of camera_bench.TorchShading."""

    def __init__(self, cam, sh, lay, w, h):
        self.cam, self.sh, self.lay, self.w, self.h = cam, sh, lay, w, h
        self.shade = TorchShading(cam, sh)
        dev = "cuda"
        self.foam_c = torch.tensor(list(lay.foam_color), device=dev)[None, :]
        self.spray_c = (torch.tensor(list(lay.spray_color), device=dev) * torch.tensor(list(sh.light_color), device=dev))[None, :]
        vec = lambda a: torch.tensor(list(a), device=dev, dtype=torch.float32)
        self.pos, self.right, self.up, self.fwd = vec(cam.position), vec(cam.right), vec(cam.up), vec(cam.forward)
        half = int(lay.spray_max_half)
        o = torch.arange(-half, half + 1, device=dev)
        self.da, self.db = (t.reshape(-1) for t in torch.meshgrid(o, o, indexing="xy"))

    def water(self, hits, V, d, length):
        """The foam mixed under the fog: image (n, 3), foam (n,), z (n,), hit (n,), and col', sky(d) for the gate."""
        s, lay = self.shade, self.lay
        P, n = V[:, 0:3], hits[:, 4:7]
        z = hits[:, 3] / length
        sky_d = s.sky(d)
        I = -(s.pos - P) / torch.sqrt(_dot(s.pos - P, s.pos - P))[:, None]
        k = 2.0 * _dot(n, I)
        r = I - k[:, None] * n
        diffuse = torch.clamp_min(_dot(n, s.L), 0.0) * 0.3
        sp = torch.clamp_min(_dot(r, s.L), 0.0)
        for _ in range(5):
            sp = sp * sp
        light = (diffuse + 0.5) + sp * 0.5
        scatter = torch.clamp_min(P[:, 1] * 0.1, 0.0)
        col = ((light[:, None] * s.wave_c) * s.sky(r)) + scatter[:, None] * s.scatter_c
        foam = V[:, 7]
        wgt = torch.clamp((foam - lay.foam_lo) / (lay.foam_hi - lay.foam_lo), 0.0, 1.0)
        wgt = ((wgt * wgt) * (3.0 - 2.0 * wgt)) * lay.foam_opacity
        col = col * (1.0 - wgt)[:, None] + ((diffuse + 0.5)[:, None] * self.foam_c) * wgt[:, None]
        f = torch.clamp_min(1.0 - torch.exp(-((z - s.fog_begin) * s.fog_density)), 0.0)
        out = col * (1.0 - f)[:, None] + sky_d * f[:, None]
        hit = hits[:, 12] == 0
        return (torch.where(hit[:, None], out, sky_d), torch.where(hit, foam, torch.zeros_like(foam)), z, hit,
                torch.where(hit[:, None], col, torch.zeros_like(col)), sky_d)

    def spray(self, rec, base, z_water, hit, sky_d):
        """Splat and composite: (image (n, 3), key int64 (n,), count int32 (n,), and sc for the gate)."""
        cam, lay, w, h = self.cam, self.lay, self.w, self.h
        T = float(np.float32(cam.tan_half_fov_y))
        e = rec[:, :3] - self.pos[None, :]
        z = _dot(e, self.fwd[None, :])
        x = _dot(e, self.right[None, :])
        y = _dot(e, self.up[None, :])
        ci = torch.floor(((x / (z * ((w / h) * T))) + 1.0) * (0.5 * w))
        cj = torch.floor((1.0 - (y / (z * T))) * (0.5 * h))
        half = torch.clamp_max(torch.floor(lay.spray_radius / (z * ((2.0 * T) / h))), float(lay.spray_max_half))
        keep = (z >= cam.near_plane) & (z <= cam.far_plane)
        a = ci[:, None] + self.da[None, :]
        b = cj[:, None] + self.db[None, :]
        ok = keep[:, None] & (self.da.abs()[None, :] <= half[:, None]) & (self.db.abs()[None, :] <= half[:, None])
        ok &= (a >= 0) & (a <= w - 1) & (b >= 0) & (b <= h - 1)
        q = (b * w + a).long().clamp_(0, w * h - 1)
        ok &= ~hit[q] | (z[:, None] < z_water[q])
        key = (z.view(torch.int32).long() << 32) | torch.arange(rec.shape[0], device="cuda")
        q, keys = q[ok], key[:, None].expand(-1, self.da.numel())[ok]
        best = torch.full((w * h,), torch.iinfo(torch.int64).max, device="cuda", dtype=torch.int64)
        best.scatter_reduce_(0, q, keys, "amin")
        count = torch.zeros((w * h,), device="cuda", dtype=torch.int32)
        count.scatter_add_(0, q, torch.ones_like(q, dtype=torch.int32))
        covered = count > 0
        zs = torch.where(covered, (best >> 32).int().view(torch.float32), torch.zeros((), device="cuda"))
        alpha = torch.clamp_max(count.float() * lay.spray_opacity, 1.0)
        s = self.shade
        fs = torch.clamp_min(1.0 - torch.exp(-((zs - s.fog_begin) * s.fog_density)), 0.0)
        sc = self.spray_c * (1.0 - fs)[:, None] + sky_d * fs[:, None]
        out = torch.where(covered[:, None], base * (1.0 - alpha)[:, None] + sc * alpha[:, None], base)
        return out, best, count, sc


def bench(timer, sampler, w, h, record_counts, say):
    cam, sh, march = default_camera(), default_shading(), default_march()
    foam_on, spray_only = default_camera_layers(), default_camera_layers(foam_opacity=0.0)
    n = w * h
    image, aux, aux2, image8 = DeviceBuffer(n * 16), DeviceBuffer(n * 16), DeviceBuffer(n * 16), DeviceBuffer(n * 4)
    scratch = DeviceBuffer(camera_layers_scratch_bytes(w, h))

    def plain():
        sampler.render(cam, sh, march, w, h, image.ptr, aux.ptr, image8.ptr)

    def layered(lay, rec=None, count=0):
        sampler.render_layers(cam, sh, march, lay, w, h, image.ptr, aux.ptr, aux2.ptr, image8.ptr,
                              records_ptr=rec.data_ptr() if rec is not None else 0, max_records=count,
                              scratch_ptr=scratch.ptr)

    # ---- foam on against ocean_camera_render ----
    layered(foam_on)
    torch.cuda.synchronize()
    a2 = aux2.to_host((n, 4))
    st = aux.to_host((n, 4))[:, 3]
    hit = st == 0
    wref = np.clip((a2[:, 0] - foam_on.foam_lo) / (foam_on.foam_hi - foam_on.foam_lo), 0, 1)
    say(f"{w} x {h} ({n} pixels, {int(hit.sum())} hit the water; foam > foam_lo on {int((wref[hit] > 0).sum())} of them, "
        f"full on {int((wref[hit] >= 1).sum())})")
    res = timer.alternating({"plain": plain, "foam": lambda: layered(foam_on)})
    p, f = res["plain"], res["foam"]
    say(f"    ocean_camera_render, image + aux + image8        {p[0]:.4f} ms ({p[1]:.4f}..{p[2]:.4f})")
    say(f"    layered, foam on, image + aux + aux2 + image8    {f[0]:.4f} ms ({f[1]:.4f}..{f[2]:.4f}) = "
        f"{f[0] / p[0]:.3f} x, {n / (f[0] * 1e-3):.3e} pixels/s")

    # ---- the spray pass: one record against N records, spread and dense ----
    saved = mips_bench.WARMUP, mips_bench.CALLS, mips_bench.ROUNDS
    one = record_list(cam, w, h, 1, False, 1)
    try:
        for count in record_counts:
            mips_bench.WARMUP, mips_bench.CALLS, mips_bench.ROUNDS = (1, 3, 3) if count > 100000 else saved
            lists = {"spread": record_list(cam, w, h, count, False, 2), "dense": record_list(cam, w, h, count, True, 3),
                     "sorted": record_list(cam, w, h, count, True, 3, ordered=True)}
            legs = {"one": lambda: layered(spray_only, one, 1)}
            for name, rec in lists.items():
                legs[name] = (lambda r: lambda: layered(spray_only, r, count))(rec)
            res = timer.alternating(legs)
            t1 = res["one"][0]
            stats = {}
            for name in lists:
                layered(spray_only, lists[name], count)
                torch.cuda.synchronize()
                c = aux2.to_host((n, 4))[:, 2].view(np.uint32)
                stats[name] = (int((c > 0).sum()), int(c.max()), int(c.astype(np.int64).sum()))
            say(f"    {count} records: water + composite with one record {t1:.4f} ms")
            for name in lists:
                t = res[name]
                dt = max(t[0] - t1, 1e-6)
                px, most, adds = stats[name]
                say(f"        {name:6s} {t[0]:.4f} ms ({t[1]:.4f}..{t[2]:.4f}): splat {dt:.4f} ms = "
                    f"{count / (dt * 1e-3):.3e} records/s, {adds / (dt * 1e-3):.3e} min + add pairs/s; "
                    f"{px} pixels covered, most hits on one {most}")
            ds = max(res["dense"][0] - t1, 1e-6) / max(res["spread"][0] - t1, 1e-6)
            so = max(res["sorted"][0] - t1, 1e-6) / max(res["spread"][0] - t1, 1e-6)
            say(f"        dense / spread (the cost of contention) = {ds:.2f}; sorted / spread (what the merge within "
                f"the wave leaves of it) = {so:.2f}")
            del lists, legs
    finally:
        mips_bench.WARMUP, mips_bench.CALLS, mips_bench.ROUNDS = saved

    # ---- composed: raycast + sample_foam + torch shading + torch scatter ----
    rays_host = camera_rays_host(cam, w, h)
    _, length_host = CR.camera_rays(cam, w, h)
    rays = DeviceBuffer.from_array(rays_host)
    hits_buf = DeviceBuffer(n * 64)
    r = torch.as_tensor(_DevicePtr(rays.ptr, (n, 8)), device="cuda")
    hits = torch.as_tensor(_DevicePtr(hits_buf.ptr, (n, 16)), device="cuda")
    length = torch.tensor(length_host, device="cuda")
    base_pts = torch.empty((n, 2), device="cuda")
    V = torch.empty((n, 8), device="cuda")
    tl = TorchLayers(cam, sh, foam_on, w, h)
    kw = dict(step=march.step, max_steps=march.max_steps, refine=march.refine, iterations=march.iterations,
              tolerance=march.tolerance, slope=march.slope, pad=march.pad)
    ok = True
    for count in [c for c in record_counts if c <= 1000000]:
        rec = record_list(cam, w, h, count, False, 2)

        def composed():
            sampler.raycast(rays.ptr, n, hits_buf.ptr, **kw)
            torch.stack((hits[:, 8], hits[:, 10]), 1, out=base_pts)
            sampler.sample_foam_device(base_pts.data_ptr(), n, V.data_ptr())
            base, foam, z, hit_t, colp, sky_d = tl.water(hits, V, r[:, 4:7], length)
            out, best, cnt, sc = tl.spray(rec, base, z, hit_t, sky_d)
            return out, best, cnt, base, colp, sky_d, sc, foam

        layered(foam_on, rec, count)
        out, best, cnt, base, colp, sky_d, sc, foam = composed()
        torch.cuda.synchronize()
        got = torch.as_tensor(_DevicePtr(image.ptr, (n, 4)), device="cuda")
        got2 = torch.as_tensor(_DevicePtr(aux2.ptr, (n, 4)), device="cuda")
        same_c = bool((got2[:, 2].view(torch.int32) == cnt).all())
        rid = torch.where(cnt > 0, (best & 0xFFFFFFFF).int(), torch.full_like(cnt, -1))
        same_r = bool((got2[:, 3].view(torch.int32) == rid).all())
        same_f = bool((got2[:, 0] == foam).all())
        bound = GATE * (colp.abs() + 2.0 * sky_d.abs() + tl.spray_c.abs()).double() + \
            2.0 ** -22 * (base.abs() + sc.abs()).double()
        diff = (got[:, :3].double() - out.double()).abs()
        within = bool((diff <= bound).all())
        ok = ok and same_c and same_r and same_f and within
        say(f"    composed, {count} spread records: counts equal {same_c}, indices equal {same_r}, foam equal {same_f}, "
            f"picture within the gate {within} (worst |a - b| / bound {float((diff / bound).max()):.3f})")
        res = timer.alternating({"layered": lambda: layered(foam_on, rec, count), "composed": composed})
        a, b = res["layered"], res["composed"]
        say(f"        layered (foam + spray, three launches) {a[0]:.4f} ms ({a[1]:.4f}..{a[2]:.4f}); composed "
            f"{b[0]:.4f} ms ({b[1]:.4f}..{b[2]:.4f}); composed / layered = {b[0] / a[0]:.2f}")
        del rec
    for buf in (rays, hits_buf, image, aux, aux2, image8, scratch):
        buf.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1025x1025")
    ap.add_argument("--records", default="10000,1000000,16000000")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "camera_layers_bench.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    timer = Timer()
    say(f"HIP events, median (min..max) of {mips_bench.ROUNDS} alternating windows of {mips_bench.CALLS} calls after "
        f"{mips_bench.WARMUP} warm-ups (record lists above 1e5: 3 windows of 3 calls after 1); 3 x 256^2 cascades, "
        f"{FOAM_STEPS} foam steps of dt {FOAM_DT}, ocean_default_camera / _shading / _march / _camera_layers")
    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.BuildBounds()
        for _ in range(FOAM_STEPS):
            g.AdvanceFoam(FOAM_DT)
        gens.append(g)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    counts = [int(v) for v in args.records.split(",")]
    ok = True
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        ok = bench(timer, sampler, w, h, counts, say) and ok
    fft.synchronize()
    for g in gens:
        g.close()
    fft.close()
    log.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
