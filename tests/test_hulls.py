"""ocean_hulls: net wave force and torque on batches of floating bodies, against the contract restated in
numpy float32 (tests/hull_loads_ref.py, on surface_query_ref and rates_ref).

Scenes as in test_surface_query.py: WaveApp's three cascades (planes 5 / 17 / 101 m), N = 64, t = 1; "calm"
is the default settings, "steep" has displacement = 1 and scale = 2. The CPU tests pin the reference itself
(on the oracle's maps and on closed forms); the GPU tests compare the kernel with the reference on the GPU's
own maps with np.array_equal: the summation order is part of the contract.

The bound of the closed-form checks, derived here and not from any result: a body's sum is a radix-64 tree of
fp32 additions. A value's path to the root passes 6 additions per level; additions of the +0.0f padding are
exact, so for up to 2 * 64 * 64 = 8192 values at most 6 + 6 + 1 = 13 additions on a path round. Each rounds
by at most u = 2^-24 relative to its result, so the computed sum differs from the exact sum of the computed
terms by at most ((1 + u)^13 - 1) * sum|a_i|. A term itself carries at most 3 roundings relative to its
closed form (the buoyancy chain rho_g * (volume * s) + drag: two products and one sum; volume * s alone: one).
Together, to first order and with the second-order part far below one unit of the 16 allowed:
|sum - closed form| <= (13 + 3) * 2^-24 * sum|a_i|.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import hull_loads_ref as H
import rates_ref
from surface_query_ref import surface_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
STEEP = dict(displacement=1.0, scale=2.0)
RHO_G = 9810.0
FOLD_BOUND = (13 + 3) * 2.0 ** -24  # times sum|a_i| (module docstring)
COUNTS = (1, 7, 31, 32, 33, 63, 64, 65, 255, 257)
F = np.float32


def _random_points(rng, n):
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = rng.uniform(-1.0, 1.0, (n, 3)) * (2.0, 0.6, 4.0)
    pts[:, 3] = rng.uniform(0.01, 0.1, n)
    pts[:, 4] = rng.uniform(0.05, 0.3, n)
    pts[:, 5] = rng.uniform(0.0, 50.0, n)
    pts[:, 6] = rng.uniform(0.0, 20.0, n)
    return pts


def _random_poses(rng, bodies, y=(-0.6, 0.6)):
    """Random rigid poses (rotations from a QR factorisation), velocities and spins."""
    out = np.zeros((bodies, 20), F)
    for b in range(bodies):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[b] = H.pose(q, (rng.uniform(-150, 150), rng.uniform(*y), rng.uniform(-150, 150)),
                        rng.uniform(-2.0, 2.0, 3), rng.uniform(-0.5, 0.5, 3))
    return out


def _bodies():
    """The hulls of the calm / steep tests: a 257-point and a 65-point hull; bodies of every count in COUNTS,
    the small ones on overlapping ranges of the second hull, plus two further instances of whole hulls."""
    rng = np.random.default_rng(21)
    points = _random_points(rng, 257 + 65)
    ranges = []
    for n in COUNTS:
        if n > 65:
            ranges.append((0, n))  # 255 and 257 share the first hull's start
        else:
            ranges.append((257 + (65 - n if n % 2 else 0), n))  # odd counts end at the hull's end, even start it
    ranges += [(0, 257), (257, 65)]
    ranges = np.array(ranges, np.int32)
    return points, ranges, _random_poses(rng, len(ranges))


def _oracle_scene(oracle, n, t=1.0, **overrides):
    """[(height, disp, jac, planeSize, displacement)] of the oracle's maps at time t."""
    cas = []
    for L in PLANES:
        g = oracle.OracleGenerator(n, oracle.default_settings(planeSize=L, **overrides))
        g.calculate_ocean(t, True)
        cas.append((g.height, g.disp, g.jac, L, g.settings.displacement))
    return cas


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# ---- without a GPU ----------------------------------------------------------------------------
def _create(L, points, n_points, ranges, bodies, fft=True, out=True):
    """ocean_hulls_create with a stand-in for the plan (the argument checks come before any use of it)."""
    h = ctypes.c_void_p()
    plan = ctypes.create_string_buffer(4096)
    rc = L.ocean_hulls_create(ctypes.byref(h) if out else None, ctypes.addressof(plan) if fft else None,
                              None if points is None else points.ctypes.data, ctypes.c_int64(n_points),
                              None if ranges is None else ranges.ctypes.data, bodies)
    assert not h.value
    return rc, L.ocean_last_error()


def test_hulls_are_exported_and_reject_bad_arguments():
    from oceansimulation_amd import capi

    L = capi.lib()
    for name in ("ocean_hulls_create", "ocean_hulls_destroy", "ocean_hulls_bodies", "ocean_hulls_instance_points",
                 "ocean_hulls_loads", "ocean_debug_hulls_packing"):
        assert hasattr(L, name) and name in capi.SIGNATURES
    good = H.box_hull()
    one = np.array([[0, 64]], np.int32)

    def bad_point(slot, value):
        p = good.copy()
        p[17, slot] = value
        return p

    cases = {
        "null out": dict(points=good, ranges=one, bodies=1, out=False),
        "null fft": dict(points=good, ranges=one, bodies=1, fft=False),
        "null points": dict(points=None, ranges=one, bodies=1),
        "null ranges": dict(points=good, ranges=None, bodies=1),
        "no bodies": dict(points=good, ranges=one, bodies=0),
        "too many bodies": dict(points=good, ranges=one, bodies=1048577),
        "count 0": dict(points=good, ranges=np.array([[0, 0]], np.int32), bodies=1),
        "count above 262144": dict(points=good, ranges=np.array([[0, 262145]], np.int32), bodies=1),
        "range past the end": dict(points=good, ranges=np.array([[0, 64], [1, 64]], np.int32), bodies=2),
        "negative first": dict(points=good, ranges=np.array([[-1, 8]], np.int32), bodies=1),
        "nan coordinate": dict(points=bad_point(1, np.nan), ranges=one, bodies=1),
        "infinite volume": dict(points=bad_point(3, np.inf), ranges=one, bodies=1),
        "nan padding": dict(points=bad_point(7, np.nan), ranges=one, bodies=1),
        "negative volume": dict(points=bad_point(3, -1.0), ranges=one, bodies=1),
        "zero half height": dict(points=bad_point(4, 0.0), ranges=one, bodies=1),
        "negative linear drag": dict(points=bad_point(5, -1.0), ranges=one, bodies=1),
        "negative quadratic drag": dict(points=bad_point(6, -1.0), ranges=one, bodies=1),
    }
    for name, kw in cases.items():
        rc, err = _create(L, kw["points"], 64, kw["ranges"], kw["bodies"], kw.get("fft", True), kw.get("out", True))
        assert rc == capi.OCEAN_ERR_INVALID and b"ocean_hulls_create" in err, (name, rc, err)
    rc = L.ocean_hulls_loads(None, None, None, 0, None, ctypes.c_float(RHO_G), 8, ctypes.c_float(0.0), 0, None, None)
    assert rc == capi.OCEAN_ERR_INVALID and b"ocean_hulls_loads" in L.ocean_last_error()
    assert L.ocean_hulls_bodies(None) == 0 and L.ocean_hulls_instance_points(None) == 0
    assert L.ocean_hulls_destroy(None) == capi.OCEAN_OK


def test_reference_on_flat_water(oracle):
    """scale = 0: the oracle's maps are flat water at eta = 0. A level 4 x 4 x 4 box with its centre at y = 0
    floats half submerged: volume, buoyancy and the vanishing torques within the derived bound; rolled by
    0.2 rad about z the torque about z restores."""
    cas = _oracle_scene(oracle, 64, scale=0.0)
    assert all(np.all(h[..., 0] == 0.0) for h, _, _, _, _ in cas)
    hull = H.box_hull(size=(2.2, 0.9, 4.3))
    ranges = np.array([[0, 64], [0, 64]], np.int32)
    poses = np.stack([H.pose(c=(3.0, 0.0, -7.0)), H.pose(_rot_z(0.2), c=(3.0, 0.0, -7.0))])
    loads, pts, info = H.hull_loads(oracle, cas, None, hull, ranges, poses, RHO_G, 8, 0.0, False)
    a = np.abs(info["a"][:64].astype(np.float64)).sum(0)
    half = float(hull[:, 3].astype(np.float64).sum()) / 2.0
    print(f"flat water: volume {loads[0, 3]} (half {half}), lift {loads[0, 1]}, torque {loads[0, 4:7]}, "
          f"bounds {FOLD_BOUND * a[[3, 1, 4, 6]]}")
    assert abs(float(loads[0, 3]) - half) <= FOLD_BOUND * a[3]
    assert abs(float(loads[0, 1]) - RHO_G * half) <= FOLD_BOUND * a[1]
    assert abs(float(loads[0, 4])) <= FOLD_BOUND * a[4] and abs(float(loads[0, 6])) <= FOLD_BOUND * a[6]
    assert loads[0, 0] == 0.0 and loads[0, 2] == 0.0 and loads[0, 7] == 32.0
    assert np.array_equal(pts[:64, 7], (hull[:, 1] < 0).astype(F))
    assert loads[1, 6] < 0.0 < loads[1, 3]  # rolled by +0.2 rad about z: the torque about z is negative


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097])
def test_reference_tree_sum(n):
    a = np.random.default_rng(n).standard_normal((n, 2)).astype(F) * F(100.0)
    a[:, 1] = np.abs(a[:, 1])
    got = H.tree_sum(a).astype(np.float64)
    want = a.astype(np.float64).sum(0)
    bound = FOLD_BOUND * np.abs(a.astype(np.float64)).sum(0)
    print(f"n = {n}: error {np.abs(got - want)}, bound {bound}")
    assert np.all(np.abs(got - want) <= bound)
    if n <= 64:  # one fold, written out: the pairwise order of the padded array
        pad = np.zeros((64, 2), F)
        pad[:n] = a
        while pad.shape[0] > 1:
            pad = pad[:pad.shape[0] // 2] + pad[pad.shape[0] // 2:]
        assert np.array_equal(H.tree_sum(a), pad[0])


def test_reference_steep_scene_mixes_cases(oracle):
    """What the GPU test on the steep scene must cover, asserted on the reference over the oracle's maps: wet,
    dry and partly wet points, and queries that stop on the tolerance as well as queries that reach the cap."""
    cas = _oracle_scene(oracle, 64, **STEEP)
    points, ranges, poses = _bodies()
    loads, pts, info = H.hull_loads(oracle, cas, None, points, ranges, poses, RHO_G, 16, 1e-4, False)
    s, used = info["s"], info["used"]
    print(f"steep reference: dry {(s == 0).sum()}, partly wet {((s > 0) & (s < 1)).sum()}, wet {(s == 1).sum()}, "
          f"stopped early {(used < 16).sum()}, at the cap {(used == 16).sum()}")
    assert (s == 0).any() and (s == 1).any() and ((s > 0) & (s < 1)).any()
    assert (used < 16).any() and (used == 16).any()
    assert np.array_equal(loads[:, 7], [float((s[a:b] > 0).sum()) for a, b in zip(info["offsets"], info["offsets"][1:])])


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _scene(ocean, n, **overrides):
    """Three generators on one plan with their rates; (sampler, host maps, host rate maps)."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(n)
    gens = []
    for plane in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=plane, **overrides)
        g.CalculateOcean(1.0)
        g.calculate_rates()
        gens.append(g)
    pairs = [(g, 0) for g in gens]
    return SurfaceSampler(pairs), host_cascades(pairs), [(g.height_rate_map_host(0), g.displacement_rate_map_host(0))
                                                         for g in gens]


@pytest.fixture(scope="module")
def calm64(ocean):
    return _scene(ocean, 64)


def _hull_set(sampler, points, ranges):
    from oceansimulation_amd.surface import HullSet

    return HullSet(sampler.fft, points, ranges)


def _check(oracle, scene, points, ranges, poses, iterations, tolerance, velocity, hulls=None):
    """One call against the reference, bit for bit; returns (loads, point_out, info of the reference)."""
    sampler, host, rates = scene
    hulls = hulls or _hull_set(sampler, points, ranges)
    loads, pts = hulls.loads_host(sampler, poses, RHO_G, iterations, tolerance, velocity)
    want_loads, want_pts, info = H.hull_loads(oracle, host, rates, points, ranges, poses, RHO_G, iterations, tolerance,
                                              velocity)
    assert np.array_equal(pts, want_pts), np.max(np.abs(pts - want_pts))
    assert np.array_equal(loads, want_loads), np.max(np.abs(loads - want_loads))
    return loads, pts, info


@pytest.mark.gpu
@pytest.mark.parametrize("velocity", [False, True])
def test_calm_scene_bit_exact(ocean, oracle, calm64, velocity):
    sampler = calm64[0]
    points, ranges, poses = _bodies()
    loads, pts, info = _check(oracle, calm64, points, ranges, poses, 8, 0.0, velocity)
    assert np.array_equal(ranges[:len(COUNTS), 1], COUNTS) and np.array_equal(ranges[-2], ranges[9])
    # the library's own query and velocity at the same world points
    q = np.ascontiguousarray(info["x"][:, [0, 2]])
    Q = sampler.query_host(q, 8, 0.0)
    assert np.array_equal(pts[:, :4], Q[:, [0, 1, 2, 7]])
    if velocity:
        assert np.array_equal(info["u"], sampler.velocity_host(np.ascontiguousarray(pts[:, [0, 2]]))[:, 4:7])
        assert np.any(info["u"] != 0.0)
    s = pts[:, 7]
    print(f"calm, water velocity {velocity}: dry {(s == 0).sum()}, partly wet {((s > 0) & (s < 1)).sum()}, "
          f"wet {(s == 1).sum()}; |F| max {np.abs(loads[:, :3]).max():.4g} N")
    assert (s == 0).any() and (s == 1).any() and ((s > 0) & (s < 1)).any()


@pytest.mark.gpu
def test_steep_scene_bit_exact(ocean, oracle):
    points, ranges, poses = _bodies()
    _, _, info = _check(oracle, _scene(ocean, 64, **STEEP), points, ranges, poses, 16, 1e-4, True)
    assert (info["used"] < 16).any() and (info["used"] == 16).any()


@pytest.mark.gpu
def test_three_level_fold(ocean, oracle, calm64):
    """4097 points are 65 tiles: 64 + 1 partials, then 2: the smallest three-level fold; 4096 the largest two-level."""
    rng = np.random.default_rng(4097)
    points = _random_points(rng, 4097)
    ranges = np.array([[0, 4097], [1, 4096]], np.int32)
    loads, _, _ = _check(oracle, calm64, points, ranges, _random_poses(rng, 2), 8, 0.0, True)
    assert np.all(loads[:, 7] > 0)


@pytest.mark.gpu
def test_small_bodies_share_waves(ocean, oracle, calm64):
    """Consecutive bodies of at most 32 points with one segment size share a wave: full and partly filled waves
    of every segment size 1 .. 32, counts below the segment size, runs broken by larger bodies, against the
    reference, and against the same set with every body on its own waves."""
    from oceansimulation_amd import capi

    sampler = calm64[0]
    rng = np.random.default_rng(32)
    points = _random_points(rng, 96)
    counts = ([16] * 40 + [3] * 5 + [70] + [1] * 70 + [2] * 33 + list(rng.integers(9, 17, 9)) + [64] +
              list(rng.integers(17, 33, 5)) + [5, 6, 7, 8] * 4 + [33] + [4] * 17 + [32, 32, 32])
    ranges = np.array([(int(rng.integers(0, 96 - n + 1)), n) for n in counts], np.int32)
    poses = _random_poses(rng, len(counts))
    loads, pts, _ = _check(oracle, calm64, points, ranges, poses, 8, 0.0, True)
    capi.lib().ocean_debug_hulls_packing(0)
    try:
        own = _hull_set(sampler, points, ranges)
    finally:
        capi.lib().ocean_debug_hulls_packing(1)
    own_loads, own_pts = own.loads_host(sampler, poses, RHO_G, 8, 0.0, True)
    assert np.array_equal(own_loads, loads) and np.array_equal(own_pts, pts)


@pytest.mark.gpu
def test_instancing_and_replay(ocean, calm64):
    """One 100-point hull at 300 poses in one call equals 300 one-body calls; a repeated call repeats its bytes."""
    sampler = calm64[0]
    rng = np.random.default_rng(300)
    points = _random_points(rng, 100)
    poses = _random_poses(rng, 300)
    many = _hull_set(sampler, points, np.tile(np.array([[0, 100]], np.int32), (300, 1)))
    loads, pts = many.loads_host(sampler, poses, RHO_G, 8, 0.0, True)
    again = many.loads_host(sampler, poses, RHO_G, 8, 0.0, True)
    assert loads.tobytes() == again[0].tobytes() and pts.tobytes() == again[1].tobytes()
    one = _hull_set(sampler, points, np.array([[0, 100]], np.int32))
    for b in range(300):
        lb, pb = one.loads_host(sampler, poses[b], RHO_G, 8, 0.0, True)
        assert lb.tobytes() == loads[b:b + 1].tobytes() and pb.tobytes() == pts[100 * b:100 * b + 100].tobytes(), b


@pytest.mark.gpu
def test_fully_dry_and_fully_wet(ocean, oracle, calm64):
    rng = np.random.default_rng(50)
    points = _random_points(rng, 200)
    ranges = np.array([[0, 200], [0, 64], [0, 200], [0, 64]], np.int32)
    poses = _random_poses(rng, 4)
    poses[:2, 10], poses[2:, 10] = 50.0, -50.0
    loads, pts, _ = _check(oracle, calm64, points, ranges, poses, 8, 0.0, True)
    assert np.all(loads[:2] == 0.0) and np.all(pts[:264, 4:] == 0.0)
    assert np.all(pts[264:, 7] == 1.0)
    assert loads[2, 3] == H.tree_sum(points[:200, 3]) and loads[3, 3] == H.tree_sum(points[:64, 3])
    assert loads[2, 7] == 200.0 and loads[3, 7] == 64.0


@pytest.mark.gpu
def test_many_points_atlas_then_direct(ocean, oracle, calm64):
    """70000 instance points on 3 x 64^2 maps take the query's atlas path; 3000 on the same plan afterwards the
    direct one."""
    sampler = calm64[0]
    rng = np.random.default_rng(70000)
    points = _random_points(rng, 250)
    poses = _random_poses(rng, 280)
    hulls = _hull_set(sampler, points, np.tile(np.array([[0, 250]], np.int32), (280, 1)))
    assert hulls.instance_points == 70000 and hulls.bodies == 280
    big, _, _ = _check(oracle, calm64, points, np.tile(np.array([[0, 250]], np.int32), (280, 1)), poses, 8, 0.0, True,
                       hulls)
    small, _, _ = _check(oracle, calm64, points, np.tile(np.array([[0, 250]], np.int32), (12, 1)), poses[:12], 8, 0.0, True)
    assert np.array_equal(small, big[:12])


@pytest.mark.gpu
def test_invalid_calls_fail_loudly(ocean):
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.slab import SlabGenerator
    from oceansimulation_amd.surface import HullSet, SurfaceSampler

    fft = ocean.FFTCalculator(64)
    gens = [ocean.Generator(fft, 1) for _ in range(2)]
    for g in gens:
        g.CalculateOcean(1.0)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    hulls = HullSet(fft, H.box_hull(), np.array([[0, 64]], np.int32))
    poses = H.pose()[None]
    gens[0].calculate_rates()
    with pytest.raises(OceanError, match="ocean_hulls_loads: generator 1 has no rates"):
        hulls.loads_host(sampler, poses, water_velocity=True)
    assert hulls.loads_host(sampler, poses, water_velocity=False)[0].shape == (1, 8)
    gens[1].calculate_rates()
    assert hulls.loads_host(sampler, poses, water_velocity=True)[0].shape == (1, 8)
    gens[0].CalculateOcean(0.25)
    with pytest.raises(OceanError, match="ocean_hulls_loads: generator 0 has stale rates"):
        hulls.loads_host(sampler, poses, water_velocity=True)
    assert hulls.loads_host(sampler, poses, water_velocity=False)[0].shape == (1, 8)
    for kw in (dict(iterations=-1), dict(iterations=65), dict(tolerance=-1.0), dict(tolerance=float("nan")),
               dict(rho_g=-1.0), dict(rho_g=float("inf"))):
        with pytest.raises(OceanError, match="ocean_hulls_loads"):
            hulls.loads_host(sampler, poses, **kw)
    with pytest.raises(OceanError, match="slab"):
        hulls.loads_host(SurfaceSampler([(SlabGenerator(ocean.FFTCalculator(256), 0, 2), 0)]), poses)
    other = ocean.Generator(ocean.FFTCalculator(128), 1)
    with pytest.raises(OceanError, match="one map size"):
        hulls.loads_host(SurfaceSampler([(gens[0], 0), (other, 0)]), poses)
    foreign = ocean.Generator(ocean.FFTCalculator(64), 1)  # the right size on another plan
    foreign.CalculateOcean(1.0)
    with pytest.raises(OceanError, match="ocean_hulls_loads: the first generator is on another plan than the hull set"):
        hulls.loads_host(SurfaceSampler([(foreign, 0)]), poses)
    with pytest.raises(OceanError, match="null poses"):
        hulls.loads(sampler, 0, 0)


@pytest.mark.gpu
def test_existing_calls_after_loads(ocean, oracle, calm64):
    """The loads share the plan's atlas and stream with the samplers: after a call on each path the forward
    sample, the query and the velocity still equal their references."""
    sampler, host, rates = calm64
    rng = np.random.default_rng(9)
    points = _random_points(rng, 250)
    xz = rng.uniform(-400.0, 400.0, (70000, 2)).astype(F)
    want_s, want_q = oracle.surface_points(host, xz), surface_query(oracle, host, xz, 4, 0.0)
    want_v = rates_ref.surface_velocity(host, rates, xz)
    for bodies, n in ((280, 70000), (8, 2000)):
        hulls = _hull_set(sampler, points, np.tile(np.array([[0, 250]], np.int32), (bodies, 1)))
        hulls.loads_host(sampler, _random_poses(rng, bodies), RHO_G, 8, 0.0, True)
        assert np.array_equal(sampler.sample_host(xz[:n].copy()), want_s[:n])
        assert np.array_equal(sampler.query_host(xz[:n].copy(), 4, 0.0), want_q[:n])
        assert np.array_equal(sampler.velocity_host(xz[:n].copy()), want_v[:n])


@pytest.mark.gpu
def test_waveapp_headless_bodies(ocean, oracle, tmp_path):
    """--bodies: the loads on the ring of box hulls the example floats equal the reference on the maps and rate
    maps it dumped."""
    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "4", "--mesh", "0", "--bodies", "16", "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    scene = json.load(open(tmp_path / "scene.json"))
    cas = [(np.load(tmp_path / f"height_{i}.npy"), np.load(tmp_path / f"disp_{i}.npy"), np.load(tmp_path / f"jac_{i}.npy"),
            c["planeSize"], c["displacement"]) for i, c in enumerate(scene["cascades"])]
    rates = [(np.load(tmp_path / f"height_rate_{i}.npy"), np.load(tmp_path / f"disp_rate_{i}.npy")) for i in range(3)]
    points, ranges = np.load(tmp_path / "hull_points.npy"), np.load(tmp_path / "hull_ranges.npy")
    poses = np.load(tmp_path / "body_poses.npy")
    got_loads, got_pts = np.load(tmp_path / "body_loads.npy"), np.load(tmp_path / "body_points.npy")
    assert points.shape == (64, 8) and ranges.shape == (16, 2) and poses.shape == (16, 20)
    assert got_loads.shape == (16, 8) and got_pts.shape == (16 * 64, 8)
    assert np.allclose(np.hypot(poses[:, 9], poses[:, 11]), 30.0, atol=1e-4)
    want_loads, want_pts, _ = H.hull_loads(oracle, cas, rates, points, ranges, poses, scene["bodies"]["rho_g"], 8, 0.0,
                                           True)
    assert np.array_equal(got_pts, want_pts) and np.array_equal(got_loads, want_loads)
    assert out["bodies"] == 16 and np.float32(out["body_max_residual"]) == got_pts[:, 3].max()
    assert np.any(got_loads[:, 3] > 0.0)
    # without the flag nothing changes
    r = subprocess.run([exe, "--n", "64", "--frames", "2", "--mesh", "0", "--probes", "8"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "bodies" not in r.stdout
