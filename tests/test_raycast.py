"""ocean_generator_build_bounds and ocean_surface_raycast: the bounds of the maps and where rays meet the
displaced water surface, against the contract restated on the oracle's forward map (tests/raycast_ref.py).

Scenes: WaveApp's three cascades (planes 5 / 17 / 101 m) at t = 1, N = 64. "Calm" is the default
settings, "steep" has displacement = 1 and scale = 2. Rays: 8192 from default_rng(17), origins uniform in
+-50 m at 2-30 m height, azimuth uniform, depression 0.5-90 degrees, tmax 400; then the first eighth starts
under water and looks up, the second eighth is horizontal near the surface, the third eighth gets a short
tmax, and half of the fourth eighth looks up from above: every status occurs. The CPU tests pin the
reference itself on the oracle's maps; the GPU tests compare the kernels with the reference on the GPU's
own maps and bounds, bit for bit.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import raycast_ref as RR
from surface_query_ref import surface_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
STEEP = dict(displacement=1.0, scale=2.0)
SCENES = {"calm": {}, "steep": STEEP}
SLOPES = (np.inf, 1.0)
PARAMS = dict(step=0.25, max_steps=256, refine=10, iterations=4, tolerance=1e-3, pad=0.0)
# |g| of the calm hits (the gap of the final evaluation at the secant point), measured on the reference
# (CPU oracle maps): 4.25e-4 m with fixed steps and 8.17e-4 m with slope 1, at a final bracket of
# 0.25 / 2^10 m: the horizontal tolerance of 1e-3 m times the local slope. The gate is 3 x that.
HIT_GAP_GATE = {np.inf: 3 * 4.25e-4, 1.0: 3 * 8.17e-4}
# Vertical rays against the cold-start query (16 iterations) at (ox, oz): the measured worst difference of
# the water height is 0. q is the same at every t, so the warm-started evaluations continue the query's own
# fixed-point sequence and stop at the same p: the gate, 3 x that, is equality.
VERTICAL_GATE = 0.0


def make_rays(n=8192):
    r = np.random.default_rng(17)
    o = np.zeros((n, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    tmax = np.full(n, 400.0, np.float32)
    o[:, 0] = r.uniform(-50, 50, n)
    o[:, 2] = r.uniform(-50, 50, n)
    o[:, 1] = r.uniform(2, 30, n)
    az = r.uniform(0, 2 * np.pi, n)
    dep = np.radians(r.uniform(0.5, 90, n))
    d[:, 0] = np.cos(dep) * np.cos(az)
    d[:, 2] = np.cos(dep) * np.sin(az)
    d[:, 1] = -np.sin(dep)
    k = n // 8
    o[:k, 1] = r.uniform(-6, -1.0, k)  # under water, looking up
    d[:k, 1] = -d[:k, 1]
    d[k:2 * k, 1] = 0  # horizontal
    d[k:2 * k, 0] = np.cos(az[k:2 * k])
    d[k:2 * k, 2] = np.sin(az[k:2 * k])
    o[k:2 * k, 1] = r.uniform(-0.5, 3, k)
    tmax[2 * k:3 * k] = r.uniform(0.5, 20, k)  # short rays
    d[3 * k:3 * k + k // 2, 1] = np.abs(d[3 * k:3 * k + k // 2, 1])  # looking up from above
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, tmax
    return rays


def _oracle_cascades(oracle, n, **overrides):
    out = []
    for L in PLANES:
        g = oracle.OracleGenerator(n, oracle.default_settings(planeSize=L, **overrides))
        g.calculate_ocean(1.0, True)
        out.append((g.height, g.disp, g.jac, L, g.settings.displacement))
    return out


@pytest.fixture(scope="module")
def cpu_runs(oracle):
    """The reference on the oracle's maps: {(scene, slope): (out, stats)} and the calm cascades."""
    rays = make_rays()
    runs, cas = {}, {}
    for name, ov in SCENES.items():
        cas[name] = _oracle_cascades(oracle, 64, **ov)
        for slope in SLOPES:
            runs[name, slope] = RR.raycast(oracle, cas[name], rays, slope=slope, with_stats=True, **PARAMS)
    return runs, cas, rays


# ---- without a GPU ----------------------------------------------------------------------------
def _raycast_rc(L, gens, cas, count=1, rays=None, n_rays=0, step=0.25, max_steps=256, refine=10, iterations=4,
                tolerance=1e-3, slope=float("inf"), pad=0.0, out=None):
    return L.ocean_surface_raycast(gens, cas, count, rays, ctypes.c_int64(n_rays), ctypes.c_float(step), max_steps,
                                   refine, iterations, ctypes.c_float(tolerance), ctypes.c_float(slope),
                                   ctypes.c_float(pad), out)


def test_exports_and_argument_checks():
    """Both calls are exported and bound, and every parameter rule of the header is refused through the
    library with its own message, before any generator is touched."""
    from oceansimulation_amd import capi

    L = capi.lib()
    for name in ("ocean_generator_build_bounds", "ocean_generator_bounds", "ocean_generator_bounds_device",
                 "ocean_surface_raycast"):
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    inv = capi.OCEAN_ERR_INVALID
    assert L.ocean_generator_build_bounds(None) == inv and b"ocean_generator_build_bounds" in L.ocean_last_error()
    buf = (ctypes.c_float * 18)()
    assert L.ocean_generator_bounds(None, 0, buf) == inv and b"ocean_generator_bounds" in L.ocean_last_error()
    assert not L.ocean_generator_bounds_device(None) and b"ocean_generator_bounds_device" in L.ocean_last_error()
    gens = (ctypes.c_void_p * 1)(None)  # one null generator: reached only when every scalar rule passes
    cas = (ctypes.c_int * 1)(0)
    one = ctypes.c_void_p(16)  # a non-null rays / out pointer that is never dereferenced
    nan, inf = float("nan"), float("inf")
    assert _raycast_rc(L, None, cas) == inv and b"null gens" in L.ocean_last_error()
    assert _raycast_rc(L, gens, None) == inv and b"null gens" in L.ocean_last_error()
    bad = [(dict(step=0.0), b"step"), (dict(step=-1.0), b"step"), (dict(step=nan), b"step"), (dict(step=inf), b"step"),
           (dict(max_steps=0), b"max_steps"), (dict(max_steps=65536), b"max_steps"),
           (dict(refine=-1), b"refine"), (dict(refine=33), b"refine"),
           (dict(iterations=-1), b"iterations"), (dict(iterations=65), b"iterations"),
           (dict(tolerance=-1e-3), b"tolerance"), (dict(tolerance=nan), b"tolerance"), (dict(tolerance=inf), b"tolerance"),
           (dict(pad=-0.5), b"pad"), (dict(pad=nan), b"pad"), (dict(pad=inf), b"pad"),
           (dict(slope=-1.0), b"slope"), (dict(slope=nan), b"slope"),
           (dict(n_rays=-1), b"negative count"), (dict(n_rays=4, rays=None, out=one), b"null rays"),
           (dict(n_rays=4, rays=one, out=None), b"null rays")]
    for kw, word in bad:
        assert _raycast_rc(L, gens, cas, **kw) == inv, kw
        assert b"ocean_surface_raycast" in L.ocean_last_error() and word in L.ocean_last_error(), (kw, L.ocean_last_error())
    # the limits themselves pass the scalar rules and reach the (null) generator
    for kw in (dict(max_steps=1), dict(max_steps=65535), dict(refine=0), dict(refine=32), dict(iterations=0),
               dict(iterations=64), dict(tolerance=0.0), dict(pad=0.0), dict(slope=0.0), dict(slope=inf),
               dict(n_rays=0), dict(n_rays=4, rays=one, out=one)):
        assert _raycast_rc(L, gens, cas, **kw) == inv, kw
        assert b"null generator" in L.ocean_last_error(), (kw, L.ocean_last_error())


def test_reference_status_mix(cpu_runs):
    """On both scenes and both slopes every status occurs at least 8 times and at least 100 hits start
    under water: the shapes the GPU tests run exercise every exit."""
    runs, _, _ = cpu_runs
    for key, (out, _) in runs.items():
        counts = np.bincount(out[:, 12].astype(int), minlength=4)
        hits_below = int(((out[:, 12] == RR.HIT) & (out[:, 13] == 1)).sum())
        print(key, "HIT/OUTSIDE/EXIT/STEP_LIMIT", counts.tolist(), "hits from below", hits_below,
              "started below", int(out[:, 13].sum()))
        assert counts.min() >= 8, (key, counts)
        assert hits_below >= 100, (key, hits_below)
        o = out[out[:, 12] == RR.OUTSIDE]
        assert np.all(o[:, :12] == 0) and np.all(o[:, 13:] == 0)


def test_reference_hits_lie_on_the_surface(cpu_runs):
    """Calm scene: the gap of every hit is within 3 x the measured worst case, and no hit keeps a
    horizontal residual above the tolerance."""
    runs, _, rays = cpu_runs
    for slope in SLOPES:
        out, _ = runs["calm", slope]
        hit = out[:, 12] == RR.HIT
        gap = float(np.abs(out[hit, 15]).max())
        share = float((out[hit, 11] > np.float32(1e-3)).mean())
        print(f"calm, slope {slope}: {hit.sum()} hits, worst |g| {gap:.3e} m, share of residuals above 1e-3: {share}")
        assert gap <= HIT_GAP_GATE[slope], (slope, gap)
        assert share == 0.0
        # row 0 is the ray at t, and t lies inside the ray's range
        t = out[hit, 3]
        assert np.array_equal(out[hit, 1], rays[hit, 1] + t * rays[hit, 5])
        assert np.all(t >= rays[hit, 3]) and np.all(t <= rays[hit, 7])


def test_reference_vertical_rays_equal_cold_query(oracle, cpu_runs):
    """An independent pin of the semantics: straight down, the water height in row 2 is the cold-start
    query's at (ox, oz), within 3 x the measured difference."""
    _, cas, _ = cpu_runs
    rng = np.random.default_rng(23)
    rays = np.zeros((1000, 8), np.float32)
    rays[:, 0], rays[:, 2] = rng.uniform(-50, 50, 1000), rng.uniform(-50, 50, 1000)
    rays[:, 1], rays[:, 5], rays[:, 7] = 10.0, -1.0, 400.0
    out = RR.raycast(oracle, cas["calm"], rays, **PARAMS)
    assert np.all(out[:, 12] == RR.HIT) and np.all(out[:, 13] == 0)
    want = surface_query(oracle, cas["calm"], rays[:, [0, 2]].copy(), 16, 1e-3)
    diff = float(np.abs(out[:, 9] - want[:, 1]).max())
    print(f"vertical rays: worst |height - cold query| {diff:.3e} m, worst |hit y - height| "
          f"{np.abs(out[:, 1] - out[:, 9]).max():.3e} m")
    assert diff <= VERTICAL_GATE
    assert np.array_equal(out[:, 0], rays[:, 0]) and np.array_equal(out[:, 2], rays[:, 2])


def test_reference_warm_start(cpu_runs):
    """Fixed-point steps per evaluation: about one on the calm scene, more where the surface folds."""
    runs, _, _ = cpu_runs
    mean = {}
    for (name, slope), (_, stats) in runs.items():
        mean[name, slope] = stats["fp_steps"] / stats["evals"]
        print(f"{name}, slope {slope}: {stats['evals']} evaluations, {mean[name, slope]:.3f} fixed-point steps each")
    for slope in SLOPES:
        assert mean["calm", slope] < mean["steep", slope]


# ---- on the GPU -------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _scene(ocean, n, **overrides):
    """Three generators on one plan with their bounds built: (sampler, host maps, host bounds (3, 18))."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(n)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L, **overrides)
        g.CalculateOcean(1.0)
        g.BuildBounds()
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


def _gen_maps(gen, c):
    return gen.height_map_host(c), gen.displacement_map_host(c), gen.jacobian_map_host(c)


def _check_bounds(gen, cascades):
    for c in range(cascades):
        want = RR.map_bounds([_gen_maps(gen, c)])[0].reshape(9, 2)
        assert np.array_equal(gen.GetBounds(c), want), c


@gpu
@pytest.mark.parametrize("n,cascades", [(16, 3), (64, 3), (256, 3), (1024, 1)])
def test_bounds_equal_numpy(ocean, n, cascades):
    """N = 16: one clamped 2048-texel item per cascade; 64: two; 256: 32; 1024: 512 (the half-spectrum frame)."""
    from oceansimulation_amd.capi import OceanError

    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=PLANES[c])
    gen.CalculateOcean(1.0)
    gen.BuildBounds()
    _check_bounds(gen, cascades)
    table = ocean.hip.to_host(gen.bounds_device(), (cascades, 18))
    assert np.array_equal(table, np.stack([gen.GetBounds(c).reshape(18) for c in range(cascades)]))
    gen.CalculateOcean(0.5)  # the maps are rewritten: stale
    with pytest.raises(OceanError, match="stale"):
        gen.GetBounds(0)
    with pytest.raises(OceanError, match="stale"):
        gen.bounds_device()
    gen.BuildBounds()
    _check_bounds(gen, cascades)
    gen.close()
    fft.close()


@gpu
def test_bounds_refused_without_a_frame_and_on_slabs(ocean):
    from oceansimulation_amd import capi
    from oceansimulation_amd.slab import SlabGenerator

    fft = ocean.FFTCalculator(64)
    gen = ocean.Generator(fft, 1)
    with pytest.raises(capi.OceanError, match="no frame"):
        gen.BuildBounds()
    with pytest.raises(capi.OceanError, match="never built"):
        gen.GetBounds(0)
    gen.CalculateOcean(1.0)
    with pytest.raises(capi.OceanError, match="never built"):
        gen.bounds_device()
    slab = SlabGenerator(ocean.FFTCalculator(256), 0, 2)
    assert capi.lib().ocean_generator_build_bounds(slab.handle) == capi.OCEAN_ERR_INVALID
    assert b"slab" in capi.lib().ocean_last_error()


@gpu
@pytest.mark.parametrize("slope", SLOPES, ids=["fixed", "slope1"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_raycast_bit_exact(ocean, oracle, scenes, scene, slope):
    sampler, host, bounds = scenes[scene]
    rays = make_rays()
    got = sampler.raycast_host(rays, slope=slope, **PARAMS)
    want = RR.raycast(oracle, host, rays, slope=slope, bounds=bounds, **PARAMS)
    counts = np.bincount(want[:, 12].astype(int), minlength=4)
    print(scene, slope, "HIT/OUTSIDE/EXIT/STEP_LIMIT", counts.tolist())
    assert counts.min() >= 8
    assert _same(got, want), np.nanmax(np.abs(got - want))


@gpu
@pytest.mark.parametrize("change", [dict(refine=0), dict(iterations=0), dict(max_steps=1), dict(pad=0.5)],
                         ids=["refine0", "iterations0", "max_steps1", "pad0.5"])
def test_raycast_parameter_edges(ocean, oracle, scenes, change):
    sampler, host, bounds = scenes["calm"]
    rays = make_rays()[::4].copy()
    kw = dict(PARAMS, slope=1.0)
    kw.update(change)
    got = sampler.raycast_host(rays, **kw)
    want = RR.raycast(oracle, host, rays, bounds=bounds, **kw)
    assert _same(got, want), np.nanmax(np.abs(got - want))
    assert sampler.raycast_host(np.zeros((0, 8), np.float32)).shape == (0, 16)


@gpu
def test_raycast_batched_generator_equals_three_generators(ocean, scenes):
    from oceansimulation_amd.surface import SurfaceSampler

    sampler, _, _ = scenes["calm"]
    gb = ocean.Generator(sampler.fft, 3)
    for c, L in enumerate(PLANES):
        ocean.apply_settings(gb.GetOceanSettings(c), planeSize=L)
    gb.CalculateOcean(1.0)
    gb.BuildBounds()
    rays = make_rays()[::8].copy()
    batched = SurfaceSampler([(gb, c) for c in range(3)]).raycast_host(rays, slope=1.0, **PARAMS)
    assert np.array_equal(batched, sampler.raycast_host(rays, slope=1.0, **PARAMS), equal_nan=True)


@gpu
def test_raycast_non_finite_rays_return(ocean, oracle, scenes):
    """NaN / inf entries and a zero direction follow the arithmetic: the call returns, equals the reference
    where that is a number and is NaN where it is NaN."""
    sampler, host, bounds = scenes["calm"]
    base = make_rays()[4096:4096 + 9 * 8].copy()  # plain rays from above
    nan, inf = np.float32("nan"), np.float32("inf")
    for k, v in enumerate((nan, inf, -inf)):
        for slot in range(8):
            base[(3 * slot + k) % len(base), slot] = v
    zero = make_rays()[4096:4104].copy()
    zero[:, 4:7] = 0.0
    zero[4:, 1] = 0.1  # inside the slab: marches in place to the step limit
    zero[6:, 7] = inf
    rays = np.concatenate([base, zero])
    for slope in SLOPES:
        kw = dict(PARAMS, slope=slope, max_steps=32)
        got = sampler.raycast_host(rays, **kw)
        want = RR.raycast(oracle, host, rays, bounds=bounds, **kw)
        assert _same(got, want), (slope, got, want)


@gpu
def test_raycast_stale_bounds_name_the_generator(ocean):
    from oceansimulation_amd.capi import OceanError

    sampler, _, _ = _scene(ocean, 64)
    rays = make_rays()[:16].copy()
    g1 = sampler.pairs[1][0]
    g1.CalculateOcean(0.0)
    with pytest.raises(OceanError, match="generator 1 has stale bounds"):
        sampler.raycast_host(rays)
    g1.BuildBounds()
    assert sampler.raycast_host(rays).shape == (16, 16)


# ---- the item loops under a CU budget ----------------------------------------------------------------
def _max_resident(wg):
    return min(32, 2048 // wg)


def _bound_holds(wg, items, budget):
    """tests/test_item_loops.py's condition: some workgroup of a budgeted grid runs three or more items."""
    return items >= 3 * budget * _max_resident(wg)


def _fill(ptr, values):
    import torch

    from oceansimulation_amd import hip

    t = torch.from_numpy(values).cuda()
    torch.cuda.synchronize()
    hip.copy_d2d(int(ptr), t.data_ptr(), values.nbytes)
    hip.synchronize()


@gpu
def test_budgeted_bounds_equal_full_device(ocean):
    """k_bounds_tiles: 256 threads, items = cascades * N^2 / 2048; k_bounds_fold: 1024 threads, items =
    cascades. 24 cascades of 128^2: 192 and 24 items, at least three per workgroup at budgets 1 and 3. The
    table and the partial rows are filled with (-3e38, +3e38) pairs first, so a skipped item shows."""
    n, cascades = 128, 24
    tiles = n * n // 2048
    for b in (1, 3):
        assert _bound_holds(256, cascades * tiles, b) and _bound_holds(1024, cascades, b)
    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=3.0 + 7.0 * c, seed=(100 + c, 7 * c))
    gen.CalculateOcean(1.0)
    gen.BuildBounds()
    fft.synchronize()
    full = ocean.hip.to_host(gen.bounds_device(), (cascades, 18))
    want = np.stack([RR.map_bounds([_gen_maps(gen, c)])[0] for c in range(cascades)])
    assert np.array_equal(full, want)
    sentinel = np.tile(np.array([-3e38, 3e38], np.float32), cascades * 9 * (1 + tiles))
    try:
        for b in (1, 3):
            fft.synchronize()
            _fill(gen.bounds_device(), sentinel)
            fft.set_cu_budget(b)
            gen.BuildBounds()
            fft.synchronize()
            assert np.array_equal(ocean.hip.to_host(gen.bounds_device(), (cascades, 18)), full), b
    finally:
        fft.set_cu_budget(0)
    gen.close()
    fft.close()


@gpu
def test_budgeted_raycast_equals_full_device(ocean, scenes):
    """k_surface_raycast: 256 rays per item; 24576 rays are 96 items, at least three per workgroup at
    budgets 1 and 3. Outputs filled with 0xFF bytes first."""
    from oceansimulation_amd.hip import DeviceBuffer

    sampler, _, _ = scenes["steep"]
    rays = np.tile(make_rays(), (3, 1))
    n = rays.shape[0]
    for b in (1, 3):
        assert _bound_holds(256, -(-n // 256), b)
    src = DeviceBuffer.from_array(rays)
    results = []
    try:
        for b in (0, 1, 3):
            out = DeviceBuffer(n * 64)
            _fill(out.ptr, np.full(n * 64, 0xFF, np.uint8))
            sampler.fft.set_cu_budget(b)
            sampler.raycast(src.ptr, n, out.ptr, slope=1.0, **PARAMS)
            sampler.fft.synchronize()
            results.append(out.to_host((n, 16)).view(np.uint32))
    finally:
        sampler.fft.set_cu_budget(0)
    assert np.array_equal(results[0][:8192], results[0][8192:16384])
    assert np.array_equal(results[1], results[0]) and np.array_equal(results[2], results[0])


@gpu
def test_samplers_after_raycast_are_still_bit_exact(ocean, oracle, scenes):
    sampler, host, _ = scenes["calm"]
    sampler.raycast_host(make_rays()[:1024].copy())
    xz = np.random.default_rng(13).uniform(-400.0, 400.0, (4000, 2)).astype(np.float32)
    assert np.array_equal(sampler.sample_host(xz), oracle.surface_points(host, xz))
    assert np.array_equal(sampler.query_host(xz, 8, 0.0), surface_query(oracle, host, xz, 8, 0.0))


@gpu
def test_waveapp_headless_rays(ocean, oracle, tmp_path):
    """--rays: the lidar ring the example casts equals the reference on the maps it dumped, and the bounds
    it dumped are the maps' minima and maxima."""
    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "4", "--mesh", "0", "--rays", "256", "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    scene = json.load(open(tmp_path / "scene.json"))
    cas = [(np.load(tmp_path / f"height_{i}.npy"), np.load(tmp_path / f"disp_{i}.npy"), np.load(tmp_path / f"jac_{i}.npy"),
            c["planeSize"], c["displacement"]) for i, c in enumerate(scene["cascades"])]
    rays, hits, bounds = np.load(tmp_path / "rays.npy"), np.load(tmp_path / "hits.npy"), np.load(tmp_path / "bounds.npy")
    assert rays.shape == (256, 8) and hits.shape == (256, 16) and bounds.shape == (len(cas), 18)
    assert np.array_equal(bounds, RR.map_bounds(cas))
    assert np.all(rays[:, :3] == np.float32([0.0, 10.0, 0.0])) and np.allclose(rays[:, 5], -np.sin(np.radians(5.0)), atol=1e-6)
    want = RR.raycast(oracle, cas, rays, bounds=bounds, **PARAMS)
    assert _same(hits, want)
    assert out["rays"] == 256 and out["ray_hits"] == int((hits[:, 12] == RR.HIT).sum())
