"""ocean_camera_render and ocean_camera_rays: ray-cast pixels shaded with the reference's water, sky and fog,
against the contract restated in numpy (tests/camera_ref.py).

Scenes as in tests/test_raycast.py: WaveApp's three cascades (planes 5 / 17 / 101 m) at t = 1, N = 64, "calm"
(the default settings) and "steep" (displacement = 1, scale = 2).
Cameras: A = position (0, 5, 0), pitch -12, yaw -135 degrees, 45 degree field of view, near 1, far 200, at
40 x 24 (6 tiles of 16 x 16, ragged on both sides); B = A with forward = L of the default shading at 9 x 7 (odd
sides: the centre pixel looks along forward, into the sun); C = A at 5 x 3 and 1 x 1 (a tile with fewer pixels
than one wave). March: step 0.25, 256 steps, 10 bisections, 4 iterations, tolerance 1e-3, pad 0, slope 1 and
+inf. The CPU tests pin the reference itself on the oracle's maps; the GPU tests compare the kernel with the
reference on the GPU's own maps and bounds.

The gate for fogged pixels (f > 0), per channel: |got - want| <= 2^-20 * (|col.c| + |sky(d).c|). OCML's expf is
documented to 1 ulp and the float64 exp rounded once is within 0.5 ulp, so f differs by less than
2^-22 + 2^-25 for e < 2; the four roundings of the mix add at most 4 * 2^-24 of the same magnitude. Everything
else (f == 0, or fog_density == 0) is bit for bit.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import camera_ref as CR
import raycast_ref as RR
import surface_lod_ref as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
SCENES = {"calm": {}, "steep": dict(displacement=1.0, scale=2.0)}
SLOPES = (1.0, float("inf"))
A_SIZE = (40, 24)
FOG_GATE = 2.0 ** -20
f32 = np.float32


def _cam_a(**kw):
    from oceansimulation_amd.surface import camera_pose

    args = dict(position=(0.0, 5.0, 0.0), pitch_deg=-12.0, yaw_deg=-135.0, fov_y_deg=45.0, near=1.0, far=200.0)
    args.update(kw)
    return camera_pose(**args)


def _cam_b():
    from oceansimulation_amd.surface import default_shading

    cam = _cam_a()
    L, _, _ = CR.host_constants(default_shading())
    for k in range(3):
        cam.forward[k] = float(L[k])
    return cam


def _march(slope=1.0, **kw):
    from oceansimulation_amd.surface import default_march

    return default_march(step=0.25, max_steps=256, refine=10, iterations=4, tolerance=1e-3, pad=0.0, slope=slope, **kw)


def _shading(**kw):
    from oceansimulation_amd.surface import default_shading

    return default_shading(**kw)


def _oracle_cascades(oracle, n, **overrides):
    out = []
    for L in PLANES:
        g = oracle.OracleGenerator(n, oracle.default_settings(planeSize=L, **overrides))
        g.calculate_ocean(1.0, True)
        out.append((g.height, g.disp, g.jac, L, g.settings.displacement))
    return out


@pytest.fixture(scope="module")
def cpu_refs(oracle):
    """The reference on the oracle's maps: cascades per scene and camera A's renders {(scene, slope)}."""
    cas = {name: _oracle_cascades(oracle, 64, **ov) for name, ov in SCENES.items()}
    runs = {(name, slope): CR.render(oracle, cas[name], _cam_a(), _shading(), _march(slope), *A_SIZE)
            for name in SCENES for slope in SLOPES}
    return cas, runs


# ---- without a GPU ----------------------------------------------------------------------------
def _render_rc(L, gens, cas, cam, sh, march, width=8, height=8, image=16, aux=16, image8=16, count=1):
    ref = lambda s: None if s is None else ctypes.byref(s)
    return L.ocean_camera_render(gens, cas, count, ref(cam), ref(sh), ref(march), width, height, ctypes.c_void_p(image),
                                 ctypes.c_void_p(aux), ctypes.c_void_p(image8))


def test_exports_and_argument_checks():
    """The calls are exported and bound, and every rule of the header is refused through the library with its
    own word, before any generator is touched. Fails without the feature."""
    import oceansimulation_amd as o
    from oceansimulation_amd import capi
    from oceansimulation_amd.surface import SurfaceSampler

    L = capi.lib()
    for name in ("ocean_default_camera", "ocean_default_shading", "ocean_default_march", "ocean_camera_rays",
                 "ocean_camera_render"):
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    for name in ("OceanCamera", "OceanShading", "OceanMarch", "camera_pose", "default_camera", "default_shading",
                 "default_march", "camera_rays_host"):
        assert hasattr(o, name) and name in o.__all__, name
    assert hasattr(SurfaceSampler, "render") and hasattr(SurfaceSampler, "render_host")
    inv = capi.OCEAN_ERR_INVALID
    gens = (ctypes.c_void_p * 1)(None)  # one null generator: reached only when every other rule passes
    cas = (ctypes.c_int * 1)(0)
    nan, inf = float("nan"), float("inf")

    def refused(word, cam=None, sh=None, march=None, **kw):
        cam = _cam_a() if cam is None else cam
        sh = _shading() if sh is None else sh
        march = _march() if march is None else march
        assert _render_rc(L, kw.pop("gens", gens), kw.pop("cas", cas), cam, sh, march, **kw) == inv, word
        msg = L.ocean_last_error()
        assert b"ocean_camera_render" in msg and word in msg, (word, msg)

    refused(b"null gens", gens=None)
    refused(b"null gens", cas=None)
    for which, word in (("cam", b"null camera"), ("sh", b"null shading"), ("march", b"null march")):
        args = dict(cam=_cam_a(), sh=_shading(), march=_march())
        args[which] = None
        assert _render_rc(L, gens, cas, **args) == inv and word in L.ocean_last_error(), word
    for kw in (dict(width=0), dict(width=16385), dict(height=0), dict(height=16385), dict(width=-3)):
        refused(b"width or height", **kw)
    for field in ("position", "right", "up", "forward"):
        for k in range(3):
            for v in (nan, inf, -inf):
                cam = _cam_a()
                getattr(cam, field)[k] = v
                refused(b"non-finite camera", cam=cam)
    for field in ("tan_half_fov_y", "near_plane", "far_plane"):
        for v in (nan, inf):
            cam = _cam_a()
            setattr(cam, field, v)
            refused(b"non-finite camera", cam=cam)
    for v in (0.0, -0.4):
        cam = _cam_a()
        cam.tan_half_fov_y = v
        refused(b"tan_half_fov_y", cam=cam)
    refused(b"near_plane", cam=_cam_a(near=-0.5))
    refused(b"near_plane", cam=_cam_a(near=200.0))
    refused(b"near_plane", cam=_cam_a(near=300.0))
    for v in (-1.0, nan, inf):
        refused(b"lod_scale", cam=_cam_a(lod_scale=v))
    for name, _ in capi.OceanShading._fields_:
        for v in (nan, inf):
            sh = _shading()
            if isinstance(getattr(sh, name), ctypes.Array):
                getattr(sh, name)[1] = v
            else:
                setattr(sh, name, v)
            refused(b"non-finite shading", sh=sh)
    refused(b"light_direction", sh=_shading(light_direction=(0.0, 0.0, 0.0)))
    refused(b"sun_view_angle", sh=_shading(sun_view_angle=-1.0))
    refused(b"sun_falloff_angle", sh=_shading(sun_falloff_angle=-1.0))
    refused(b"fog_density", sh=_shading(fog_density=-0.001))
    bad = [(dict(step=0.0), b"step"), (dict(step=-1.0), b"step"), (dict(step=nan), b"step"), (dict(step=inf), b"step"),
           (dict(max_steps=0), b"max_steps"), (dict(max_steps=65536), b"max_steps"),
           (dict(refine=-1), b"refine"), (dict(refine=33), b"refine"),
           (dict(iterations=-1), b"iterations"), (dict(iterations=65), b"iterations"),
           (dict(tolerance=-1e-3), b"tolerance"), (dict(tolerance=nan), b"tolerance"), (dict(tolerance=inf), b"tolerance"),
           (dict(pad=-0.5), b"pad"), (dict(pad=nan), b"pad"), (dict(pad=inf), b"pad"),
           (dict(slope=-1.0), b"slope"), (dict(slope=nan), b"slope")]
    for kw, word in bad:
        m = _march()
        for k, v in kw.items():
            setattr(m, k, v)
        refused(word, march=m)
    refused(b"outputs", image=0, aux=0, image8=0)
    # the limits themselves pass every rule and reach the (null) generator
    for kw in (dict(width=1, height=1), dict(width=16384, height=16384), dict(image=0, aux=0), dict(aux=0, image8=0),
               dict(cam=_cam_a(near=0.0)), dict(cam=_cam_a(lod_scale=1.5)), dict(sh=_shading(fog_density=0.0)),
               dict(sh=_shading(sun_view_angle=0.0, sun_falloff_angle=0.0)), dict(march=_march(slope=inf))):
        refused(b"null generator", **kw)
    # ocean_camera_rays: the camera's rules, then the output
    one = ctypes.c_void_p(16)
    assert L.ocean_camera_rays(None, 4, 4, one, None) == inv and b"null camera" in L.ocean_last_error()
    cam = _cam_a()
    assert L.ocean_camera_rays(ctypes.byref(cam), 0, 4, one, None) == inv and b"width or height" in L.ocean_last_error()
    assert L.ocean_camera_rays(ctypes.byref(cam), 4, 4, None, None) == inv and b"null rays" in L.ocean_last_error()
    cam.tan_half_fov_y = 0.0
    assert L.ocean_camera_rays(ctypes.byref(cam), 4, 4, one, None) == inv and b"tan_half_fov_y" in L.ocean_last_error()


def test_defaults_equal_the_reference_numbers():
    """src/Renderer.cpp:14-16 and src/Renderer.h:22-29; the 45 degree field of view is this library's choice."""
    from oceansimulation_amd.surface import camera_pose, default_camera, default_march, default_shading

    c = default_camera()
    want = camera_pose((0.0, 5.0, 0.0), -5.0, -135.0, 45.0, 1.0, 1500.0)
    assert bytes(c) == bytes(want)
    assert list(c.position) == [0.0, 5.0, 0.0] and c.near_plane == 1.0 and c.far_plane == 1500.0 and c.lod_scale == 0.0
    p, y = np.radians(-5.0), np.radians(-135.0)
    fwd = np.array([np.cos(p) * np.sin(y), np.sin(p), -np.cos(p) * np.cos(y)])
    right = np.array([np.cos(y), 0.0, np.sin(y)])
    assert np.array_equal(np.array(c.forward[:], f32), fwd.astype(f32))
    assert np.array_equal(np.array(c.right[:], f32), right.astype(f32))
    assert np.array_equal(np.array(c.up[:], f32), np.cross(right, fwd).astype(f32))
    assert c.tan_half_fov_y == f32(np.tan(np.radians(22.5)))
    s = default_shading()
    assert np.array_equal(np.array(s.wave_color[:], f32), f32([0.0, 0.33, 0.47]))
    assert np.array_equal(np.array(s.scatter_color[:], f32), f32([0.5, 0.8, 0.9]))
    assert np.array_equal(np.array(s.sky_color[:], f32), f32([0.53, 0.8, 0.94]))
    assert np.array_equal(np.array(s.light_color[:], f32), f32([1.0, 1.0, 1.0]))
    assert np.array_equal(np.array(s.light_direction[:], f32), f32([0.703, 0.105, 0.703]))
    assert (s.sun_view_angle, s.sun_falloff_angle, s.fog_begin) == (3.0, 1.0, 30.0) and s.fog_density == f32(0.0025)
    m = default_march()
    assert (m.step, m.max_steps, m.refine, m.iterations, m.slope, m.pad) == (0.25, 256, 10, 4, 1.0, 0.0)
    assert m.tolerance == f32(1e-3)


def test_reference_pixel_mix(cpu_refs):
    """Conditions on the reference: on A at least a quarter of the pixels hit and a quarter do not, and of the
    hits at least a tenth lie before the fog and a tenth in it, so every branch of the shading is compared."""
    _, runs = cpu_refs
    fog_begin = _shading().fog_begin
    for key, r in runs.items():
        n = r["status"].size
        hit = r["status"] == RR.HIT
        near = int((r["z"][hit] < fog_begin).sum())
        far = int((r["z"][hit] >= fog_begin).sum())
        counts = np.bincount(r["status"], minlength=4).tolist()
        print(key, "HIT/OUTSIDE/EXIT/STEP_LIMIT", counts, "hits before / in the fog", near, far)
        assert hit.sum() >= n // 4 and (~hit).sum() >= n // 4, (key, counts)
        assert near >= hit.sum() / 10 and far >= hit.sum() / 10, (key, near, far)
        assert np.all(r["f"][hit][r["z"][hit] < fog_begin] == 0) and np.all(r["f"][hit][r["z"][hit] > fog_begin] > 0)
        assert np.all(r["aux"].reshape(-1, 4)[r["status"] == RR.OUTSIDE] == f32([0, 0, 0, 1]))


def test_reference_sun_pixel(oracle, cpu_refs):
    """B: the centre pixel looks along L; the sun burns to exactly 2 * light_color, 255 in every byte."""
    cas, _ = cpu_refs
    r = CR.render(oracle, cas["calm"], _cam_b(), _shading(), _march(), 9, 7)
    centre = r["image"][3, 4]
    assert r["status"].reshape(7, 9)[3, 4] != RR.HIT
    assert np.array_equal(centre, f32([2.0, 2.0, 2.0, 1.0])), centre
    assert np.array_equal(r["image8"][3, 4], np.uint8([255, 255, 255, 255]))
    assert np.array_equal(r["rays"][3 * 9 + 4, 4:7], CR.host_constants(_shading())[0])


def test_reference_sky_fog_and_lod_identities(oracle, cpu_refs):
    """Pixels that do not hit equal sky(d); fog_density = 0 leaves col; lod_scale = 0 is the level-0 fragment
    stage (the raycast rows' normal), and a footprint below one texel of every cascade gives the same picture."""
    cas, runs = cpu_refs
    r = runs["calm", 1.0]
    miss = r["status"] != RR.HIT
    assert np.array_equal(r["image"].reshape(-1, 4)[miss, :3], r["sky_d"][miss])
    assert np.array_equal(r["sky_d"], CR.sky(r["rays"][:, 4:7], _shading()))
    clear = CR.render(oracle, cas["calm"], _cam_a(), _shading(fog_density=0.0), _march(1.0), *A_SIZE)
    hit = ~miss
    assert np.all(clear["f"] == 0) and np.array_equal(clear["image"].reshape(-1, 4)[hit, :3], clear["col"][hit])
    assert np.array_equal(clear["col"], r["col"]) and np.array_equal(clear["aux"], r["aux"])
    assert np.array_equal(r["normal"], r["hits"][:, 4:7])
    tiny = CR.render(oracle, cas["calm"], _cam_a(lod_scale=1e-4), _shading(), _march(1.0), *A_SIZE)
    assert np.array_equal(tiny["image"], r["image"]) and np.array_equal(tiny["aux"], r["aux"])


def test_reference_fp32_against_float64(cpu_refs):
    """The fp32 restatement against the float64 reading of the same shading at the same hits. Documentation
    (profiles/camera_parity.md quotes the printed figures), not the GPU gate."""
    _, runs = cpu_refs
    worst = 0.0
    for key, r in runs.items():
        hit = r["status"] == RR.HIT
        s64 = CR.shade(r["P"], r["normal"], r["rays"][:, 4:7], r["z"], hit, _cam_a().position, _shading(), np.float64)
        diff = np.abs(r["image"].reshape(-1, 4)[:, :3].astype(np.float64) - s64["out"])
        scale = np.abs(s64["col"]) + np.abs(s64["sky_d"])
        rel = float((diff / scale).max())
        print(key, f"largest |fp32 - float64| {diff.max():.3e}, relative to |col| + |sky(d)| {rel:.3e} "
                   f"({rel * 2 ** 24:.2f} x 2^-24)")
        worst = max(worst, rel)
    # sanity only: a handful of fp32 roundings per channel, far from any formula error
    assert worst < 1e-4


# ---- on the GPU -------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _scene(ocean, n, mips=False, **overrides):
    """Three generators on one plan with their bounds built: (sampler, host maps, host bounds (3, 18))."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(n)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L, **overrides)
        g.CalculateOcean(1.0)
        g.BuildBounds()
        if mips:
            g.build_mips()
        gens.append(g)
    pairs = [(g, 0) for g in gens]
    return SurfaceSampler(pairs), host_cascades(pairs), np.stack([g.GetBounds(0).reshape(18) for g in gens])


@pytest.fixture(scope="module")
def scenes(ocean):
    return {name: _scene(ocean, 64, **ov) for name, ov in SCENES.items()}


def _same(got, want):
    """Bit for bit where the reference is a number (-0 == +0), NaN where it is NaN."""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def _compare(got, ref, fogged_exact):
    """got = (image, aux, image8) of the device, ref = camera_ref.render's dict. aux everywhere, image and
    image8 on every pixel whose reference f is 0 (all of them when fogged_exact) bit for bit; the others
    within the gate."""
    image, aux, image8 = got
    h, w = image.shape[:2]
    assert _same(aux, ref["aux"]), np.nanmax(np.abs(aux - ref["aux"]))
    f = ref["f"].reshape(h, w)
    exact = np.ones((h, w), bool) if fogged_exact else f == 0
    assert _same(image[exact], ref["image"][exact]), np.abs(image[exact] - ref["image"][exact]).max()
    assert np.array_equal(image8[exact], ref["image8"][exact])
    fog = ~exact
    if fog.any():
        bound = FOG_GATE * (np.abs(ref["col"]) + np.abs(ref["sky_d"])).reshape(h, w, 3)[fog]
        diff = np.abs(image[fog][:, :3].astype(np.float64) - ref["image"][fog][:, :3].astype(np.float64))
        print(f"fogged pixels: {int(fog.sum())}, worst |got - want| / bound {float((diff / bound).max()):.3f}, "
              f"differing channels {int((diff > 0).sum())}")
        assert np.all(diff <= bound), float((diff / bound).max())
        assert np.all(image[fog][:, 3] == 1.0)
        # a byte moves by at most one step where the float moved at all
        assert np.abs(image8[fog].astype(int) - ref["image8"][fog].astype(int)).max() <= 1
    return int(fog.sum())


@gpu
@pytest.mark.parametrize("slope", SLOPES, ids=["slope1", "fixed"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_render_a_against_reference(ocean, oracle, scenes, scene, slope):
    sampler, host, bounds = scenes[scene]
    for density in (0.0, 0.0025):
        sh = _shading(fog_density=density)
        got = sampler.render_host(_cam_a(), *A_SIZE, shading=sh, march=_march(slope))
        ref = CR.render(oracle, host, _cam_a(), sh, _march(slope), *A_SIZE, bounds=bounds)
        hit = ref["status"] == RR.HIT
        assert hit.sum() >= 240 and (~hit).sum() >= 240
        fogged = _compare(got, ref, fogged_exact=density == 0.0)
        assert (fogged > 0) == (density > 0)


@gpu
def test_render_b_and_c_against_reference(ocean, oracle, scenes):
    sampler, host, bounds = scenes["calm"]
    for cam, (w, h) in ((_cam_b(), (9, 7)), (_cam_a(), (5, 3)), (_cam_a(), (1, 1))):
        for density in (0.0, 0.0025):
            sh = _shading(fog_density=density)
            got = sampler.render_host(cam, w, h, shading=sh, march=_march())
            ref = CR.render(oracle, host, cam, sh, _march(), w, h, bounds=bounds)
            _compare(got, ref, fogged_exact=density == 0.0)
    image, _, image8 = sampler.render_host(_cam_b(), 9, 7)
    assert np.array_equal(image[3, 4], f32([2.0, 2.0, 2.0, 1.0])) and np.all(image8[3, 4] == 255)


@gpu
def test_render_lod_against_reference_and_freshness(ocean, oracle):
    from oceansimulation_amd.capi import OceanError

    sampler, host, bounds = _scene(ocean, 64, mips=True)
    cam, sh = _cam_a(lod_scale=1.5), _shading(fog_density=0.0)
    got = sampler.render_host(cam, *A_SIZE, shading=sh, march=_march())
    ref = CR.render(oracle, host, cam, sh, _march(), *A_SIZE, bounds=bounds, pyramids=SL.build_pyramids(host))
    _compare(got, ref, fogged_exact=True)
    level0 = sampler.render_host(_cam_a(), *A_SIZE, shading=sh, march=_march())
    assert not np.array_equal(level0[0], got[0])  # the pyramid is in use
    assert np.array_equal(level0[1][..., [0, 1, 3]], got[1][..., [0, 1, 3]])  # the march is level 0 either way
    g1 = sampler.pairs[1][0]
    g1.CalculateOcean(0.0)  # the maps are rewritten: bounds and pyramid are stale
    with pytest.raises(OceanError, match="generator 1 has stale bounds"):
        sampler.render_host(_cam_a(), *A_SIZE)
    g1.BuildBounds()
    with pytest.raises(OceanError, match="generator 1 has a stale mip pyramid"):
        sampler.render_host(cam, *A_SIZE)
    assert sampler.render_host(_cam_a(), *A_SIZE)[0].shape == (24, 40, 4)  # lod_scale 0 never needs it
    g1.build_mips()
    assert sampler.render_host(cam, *A_SIZE)[0].shape == (24, 40, 4)
    fresh, _, _ = _scene(ocean, 64)  # never built
    with pytest.raises(OceanError, match="generator 0 has no mip pyramid"):
        fresh.render_host(cam, *A_SIZE)
    assert fresh.render_host(_cam_a(), *A_SIZE)[0].shape == (24, 40, 4)


@gpu
def test_camera_rays_and_raycast_agree_with_aux(ocean, scenes):
    from oceansimulation_amd.surface import camera_rays_host

    sampler, _, _ = scenes["steep"]
    for cam, (w, h) in ((_cam_a(), A_SIZE), (_cam_b(), (9, 7)), (_cam_a(), (1, 1)), (ocean.default_camera(), (33, 17))):
        rays = camera_rays_host(cam, w, h)
        want, length = CR.camera_rays(cam, w, h)
        assert np.array_equal(rays, want)
        _, aux, _ = sampler.render_host(cam, w, h, march=_march())
        hits = sampler.raycast_host(rays, step=0.25, max_steps=256, refine=10, iterations=4, tolerance=1e-3, slope=1.0,
                                    pad=0.0)
        aux = aux.reshape(-1, 4)
        assert _same(aux[:, [0, 2, 3]], hits[:, [3, 7, 12]])
        assert _same(aux[:, 1], (hits[:, 3] / length).astype(f32))


def _fill(ptr, values):
    import torch

    from oceansimulation_amd import hip

    t = torch.from_numpy(values).cuda()
    torch.cuda.synchronize()
    hip.copy_d2d(int(ptr), t.data_ptr(), values.nbytes)
    hip.synchronize()


@gpu
@pytest.mark.parametrize("size", [A_SIZE, (100, 68)], ids=["6tiles", "35tiles"])
def test_budgeted_render_equals_full_device(ocean, scenes, size):
    """k_camera_render: a 16 x 16 tile per item. A has 6 tiles; 100 x 68 has 35, ragged on both sides, which is
    at least three items per workgroup of the 8 resident under a budget of one CU (tests/test_item_loops.py's
    condition), so the item loop runs past its first item. Outputs filled with 0xFF bytes first; a second
    render with the full device replays the first bit for bit."""
    from oceansimulation_amd.hip import DeviceBuffer

    sampler, _, _ = scenes["steep"]
    w, h = size
    n = w * h
    results = []
    try:
        for b in (0, 1, 0):
            bufs = [DeviceBuffer(n * 16), DeviceBuffer(n * 16), DeviceBuffer(n * 4)]
            for buf, size_b in zip(bufs, (n * 16, n * 16, n * 4)):
                _fill(buf.ptr, np.full(size_b, 0xFF, np.uint8))
            sampler.fft.set_cu_budget(b)
            sampler.render(_cam_a(), _shading(), _march(), w, h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
            sampler.fft.synchronize()
            results.append([bufs[0].to_host((n, 4)).view(np.uint32), bufs[1].to_host((n, 4)).view(np.uint32),
                            bufs[2].to_host((n, 4), np.uint8)])
    finally:
        sampler.fft.set_cu_budget(0)
    for k in range(3):
        assert np.array_equal(results[1][k], results[0][k]), k  # budget 1 == full device
        assert np.array_equal(results[2][k], results[0][k]), k  # two renders are identical
    assert not np.any(results[0][2][:, 3] != 255) and np.all(results[0][0][:, 3] == f32(1.0).view(np.uint32))


@gpu
def test_null_outputs_leave_the_others_unchanged(ocean, scenes):
    from oceansimulation_amd.hip import DeviceBuffer

    sampler, _, _ = scenes["calm"]
    w, h = A_SIZE
    full = sampler.render_host(_cam_a(), w, h)
    image8 = DeviceBuffer(w * h * 4)
    sampler.render(_cam_a(), _shading(), _march(), w, h, 0, 0, image8.ptr)
    sampler.fft.synchronize()
    assert np.array_equal(image8.to_host((h, w, 4), np.uint8), full[2])
    aux = DeviceBuffer(w * h * 16)
    sampler.render(_cam_a(), _shading(), _march(), w, h, 0, aux.ptr, 0)
    sampler.fft.synchronize()
    assert np.array_equal(aux.to_host((h, w, 4)).view(np.uint32), full[1].view(np.uint32))


@gpu
def test_batched_generator_equals_three_generators(ocean, scenes):
    from oceansimulation_amd.surface import SurfaceSampler

    sampler, _, _ = scenes["calm"]
    gb = ocean.Generator(sampler.fft, 3)
    for c, L in enumerate(PLANES):
        ocean.apply_settings(gb.GetOceanSettings(c), planeSize=L)
    gb.CalculateOcean(1.0)
    gb.BuildBounds()
    batched = SurfaceSampler([(gb, c) for c in range(3)]).render_host(_cam_a(), *A_SIZE)
    for a, b in zip(batched, sampler.render_host(_cam_a(), *A_SIZE)):
        assert np.array_equal(a, b, equal_nan=a.dtype != np.uint8)


@gpu
def test_camera_under_water_returns_and_matches(ocean, oracle, scenes):
    """Position y = -3, looking up (pitch +40): rays start below the surface and hit it from below."""
    sampler, host, bounds = scenes["calm"]
    cam = _cam_a(position=(0.0, -3.0, 0.0), pitch_deg=40.0)
    sh = _shading(fog_density=0.0)
    got = sampler.render_host(cam, *A_SIZE, shading=sh, march=_march())
    ref = CR.render(oracle, host, cam, sh, _march(), *A_SIZE, bounds=bounds)
    hit = ref["status"] == RR.HIT
    assert hit.sum() >= 100 and np.all(ref["hits"][hit, 13] == 1)  # hits from below
    _compare(got, ref, fogged_exact=True)


@gpu
def test_samplers_after_render_are_still_bit_exact(ocean, oracle, scenes):
    from test_raycast import PARAMS, make_rays

    sampler, host, bounds = scenes["calm"]
    sampler.render_host(_cam_a(), *A_SIZE)
    xz = np.random.default_rng(13).uniform(-400.0, 400.0, (4000, 2)).astype(np.float32)
    assert np.array_equal(sampler.sample_host(xz), oracle.surface_points(host, xz))
    rays = make_rays()[::8].copy()
    got = sampler.raycast_host(rays, slope=1.0, **PARAMS)
    assert _same(got, RR.raycast(oracle, host, rays, slope=1.0, bounds=bounds, **PARAMS))


@gpu
def test_waveapp_headless_image(ocean, tmp_path):
    """--image 40x24 --dump: the arrays the example writes equal render_host of the default camera on the same
    scene (the example's generators rebuilt here: the dumped maps are compared first)."""
    from oceansimulation_amd.surface import SurfaceSampler

    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "3", "--mesh", "0", "--image", "40x24", "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    fft = ocean.FFTCalculator(64)
    gens = []
    for i, L in enumerate(PLANES):
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L, boundWavelength=1, wavelengthMax=L / 2.0,
                             wavelengthMin=0.0 if i == 0 else PLANES[i - 1] / 2.0)
        gens.append(g)
    for _ in range(3):
        for g in gens:
            g.CalculateOcean(float(f32(1.0) / f32(60.0)), True)
    for i, g in enumerate(gens):
        g.BuildBounds()
        assert np.array_equal(np.load(tmp_path / f"height_{i}.npy"), g.height_map_host(0)), i
        assert np.array_equal(np.load(tmp_path / f"disp_{i}.npy"), g.displacement_map_host(0)), i
    image, aux, image8 = SurfaceSampler([(g, 0) for g in gens]).render_host(ocean.default_camera(), 40, 24)
    got = [np.load(tmp_path / name) for name in ("image.npy", "image_aux.npy", "image8.npy")]
    assert got[0].shape == (24, 40, 4) and got[2].dtype == np.uint8
    assert np.array_equal(got[0], image, equal_nan=True) and np.array_equal(got[1], aux, equal_nan=True)
    assert np.array_equal(got[2], image8)
    assert out["image_hits"] == int((aux[..., 3] == 0).sum()) and out["image_hits"] > 0
