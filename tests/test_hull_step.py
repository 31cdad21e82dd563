"""ocean_hulls_step: the bodies of a hull set stepped on the device from their wave loads, against the contract
restated in numpy float32 (tests/hull_step_ref.py on tests/hull_loads_ref.py).

The CPU tests pin the restatement itself on closed forms (free fall, a torque-free spin, a box settling on flat
water) and the host's argument checks. The GPU tests compare the kernels with the restatement on the GPU's own
maps with np.array_equal: poses, loads and point_out, bit for bit. Scenes as in test_hulls.py (N = 64, three
cascades; "calm" the defaults, "steep" displacement = 1 and scale = 2).

Gates of the closed-form tests. The closed forms are those of the recurrence itself (semi-implicit Euler, the
Cayley map), so a float64 evaluation of the same recurrence on the same float32 inputs agrees with them to
1e-12; what the float32 restatement adds is its rounding. That deviation was measured once, with
hull_step_ref's dtype=float64 over the inputs of each test (the largest over the steps), is written at the
test, and the test gates at 4 times it.

The orthogonality bound, derived by counting the roundings of the Gram-Schmidt pass and not from any result
(u = 2^-24, first order; the pass runs every substep on a matrix within a few u of a rotation, so nothing
accumulates):
  row 0: |r0|^2 is three products and two sums of positive terms, relative error <= 3u; sqrtf halves that and
    adds its own u: 2.5u; each quotient adds u: a common factor within 3.5u, so | |e0|^2 - 1 | <= 7u.
  row 1: d = e0 . r1 carries <= 3u (|e0| |r1| ~ 1); u = r1 - d e0 rounds each difference by <= u |u.k| (d is
    itself a few u, so the products' roundings are second order). e0 . u = (d_exact - d) + d (1 - |e0|^2) +
    the differences' roundings <= 3u + u sum|e0.k||u.k| <= 4u, and it stays that after the common scaling by
    1 / l1. The normalisation as for row 0, plus 2u from the differences: | |e1|^2 - 1 | <= 9u.
  row 2: e2.k is two products and a difference, error <= 2u (|ab| + |cd|) <= 2u per component, <= 2 sqrt(3) u
    < 3.5u as a vector. The exact cross product has |e0 x e1|^2 = |e0|^2 |e1|^2 - (e0 . e1)^2, within 7u + 9u
    of 1, and is orthogonal to e0 and e1: | |e2|^2 - 1 | <= 16u + 2 * 3.5u = 23u, |e2 . e0|, |e2 . e1| <= 3.5u.
So every entry of R R^T - I is within 23u; the tests allow ORTHO_BOUND = 24u (R R^T evaluated in float64).
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import hull_loads_ref as H
import hull_step_ref as S
from surface_query_ref import surface_query
from test_hulls import FOLD_BOUND, RHO_G, STEEP, _oracle_scene, _random_points, _random_poses, _rot_z, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DT = 1.0 / 60.0
ORTHO_BOUND = 24 * 2.0 ** -24  # module docstring


def _ortho_error(poses):
    R = np.asarray(poses, np.float64).reshape(-1, 20)[:, :9].reshape(-1, 3, 3)
    return float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())


# ---- without a GPU ----------------------------------------------------------------------------
def test_step_is_exported_and_rejects_bad_arguments():
    """The symbols, and the calls that are refused before the hull set or a generator is touched (a stand-in
    for the set: the checks come before any use of it)."""
    from oceansimulation_amd import capi
    from oceansimulation_amd.surface import HullSet

    L = capi.lib()
    for name in ("ocean_hulls_set_bodies", "ocean_default_hull_step_settings", "ocean_hulls_step"):
        assert hasattr(L, name) and name in capi.SIGNATURES
    d = HullSet.step_settings()
    assert (d.substeps, d.iterations, d.water_velocity) == (1, 8, 0) and d.dt == F(DT) and d.tolerance == 0.0
    assert list(d.gravity) == [0.0, F(-9.8), 0.0] and d.rho_g == 9810.0
    L.ocean_default_hull_step_settings(None)  # a null pointer is ignored

    stand_in = ctypes.create_string_buffer(4096)
    hulls = ctypes.addressof(stand_in)
    props = np.stack([S.props(100.0, (10.0, 20.0, 30.0))])
    poses = ctypes.addressof(ctypes.create_string_buffer(80))
    for h, p in ((None, props.ctypes.data), (hulls, None)):
        assert L.ocean_hulls_set_bodies(h, p) == capi.OCEAN_ERR_INVALID
        assert b"ocean_hulls_set_bodies: null argument" in L.ocean_last_error()

    def step(h=hulls, settings=d, poses=poses):
        rc = L.ocean_hulls_step(h, None, None, 0, ctypes.byref(settings) if settings is not None else None, poses, None,
                                None, None)
        return rc, L.ocean_last_error()

    cases = {
        "null hull set": (dict(h=None), b"null hull set"),
        "null settings": (dict(settings=None), b"null settings/poses"),
        "null poses": (dict(poses=None), b"null settings/poses"),
        "dt 0": (dict(settings=HullSet.step_settings(dt=0.0)), b"dt must be finite and > 0"),
        "dt negative": (dict(settings=HullSet.step_settings(dt=-DT)), b"dt must be finite and > 0"),
        "dt nan": (dict(settings=HullSet.step_settings(dt=float("nan"))), b"dt must be finite and > 0"),
        "dt inf": (dict(settings=HullSet.step_settings(dt=float("inf"))), b"dt must be finite and > 0"),
        "substeps 0": (dict(settings=HullSet.step_settings(substeps=0)), b"substeps outside 1..64"),
        "substeps 65": (dict(settings=HullSet.step_settings(substeps=65)), b"substeps outside 1..64"),
        "gravity nan": (dict(settings=HullSet.step_settings(gravity=(0.0, float("nan"), 0.0))), b"gravity must be finite"),
        "gravity inf": (dict(settings=HullSet.step_settings(gravity=(float("inf"), 0.0, 0.0))), b"gravity must be finite"),
        "iterations 65": (dict(settings=HullSet.step_settings(iterations=65)), b"iterations outside 0..64"),
        "tolerance nan": (dict(settings=HullSet.step_settings(tolerance=float("nan"))), b"tolerance must be finite"),
        "rho_g negative": (dict(settings=HullSet.step_settings(rho_g=-1.0)), b"rho_g must be finite and >= 0"),
        "water_velocity 2": (dict(settings=HullSet.step_settings(water_velocity=2)), b"water_velocity must be 0 or 1"),
        "no generators": (dict(), b"ocean_hulls_step"),  # every setting valid: the request's own rules refuse it
    }
    for name, (kw, message) in cases.items():
        rc, err = step(**kw)
        assert rc == capi.OCEAN_ERR_INVALID and b"ocean_hulls_step" in err and message in err, (name, rc, err)


# the largest |float32 - float64| of the recurrence over the 200 steps of test_free_fall, measured once
FREE_FALL_DEV_V, FREE_FALL_DEV_C = 3.71e-5, 9.36e-5


def test_free_fall():
    """A body high above the water, no damping: after n steps v.y = -g h n and c.y = c0 - g h^2 n (n + 1) / 2, the
    closed forms of semi-implicit Euler, at every step up to n = 200; x, z, R and w never change."""
    n, c0 = 200, 500.0
    props = S.props(100.0, (10.0, 20.0, 30.0))[None]
    start = H.pose(c=(1.0, c0, 2.0))[None]
    g, h = float(F(9.8)), float(F(DT))
    p32, p64 = start.copy(), start.astype(np.float64)
    dev_v = dev_c = err_v = err_c = 0.0
    for i in range(1, n + 1):
        p32, _, _ = S.hull_step(S.dry_loads, p32, props, DT, 1)
        p64, _, _ = S.hull_step(S.dry_loads, p64, props, DT, 1, dtype=np.float64)
        want_v, want_c = -g * h * i, c0 - g * h * h * i * (i + 1) / 2
        assert abs(p64[0, 13] - want_v) < 1e-11 and abs(p64[0, 10] - want_c) < 1e-10  # the closed forms are the recurrence's
        dev_v, dev_c = max(dev_v, abs(float(p32[0, 13]) - p64[0, 13])), max(dev_c, abs(float(p32[0, 10]) - p64[0, 10]))
        err_v, err_c = max(err_v, abs(float(p32[0, 13]) - want_v)), max(err_c, abs(float(p32[0, 10]) - want_c))
    print(f"free fall: float32 - float64 at most {dev_v:.3e} m/s, {dev_c:.3e} m; against the closed forms {err_v:.3e}, "
          f"{err_c:.3e}; gates {4 * FREE_FALL_DEV_V:.3e}, {4 * FREE_FALL_DEV_C:.3e}")
    assert err_v <= 4 * FREE_FALL_DEV_V and err_c <= 4 * FREE_FALL_DEV_C
    assert p32.dtype == F and np.array_equal(p32[0, [9, 11, 12, 14]], start[0, [9, 11, 12, 14]])
    assert np.array_equal(p32[0, :9], start[0, :9]) and np.all(p32[0, 15:] == 0.0)


# the largest |float32 - float64| of the rotation angle over the 1000 steps of test_torque_free_spin, measured
# once per axis. About z it is larger: row 2 of R is the cross product e0 x e1, so for a spin about z the entry
# R[2][2] that carries w into the body frame and back is 1 only to a few u, and w drifts by that factor twice a
# step (3.0003 rad/s after 1000 steps); about x and y that entry is a normalised (1, 0, 0), exactly 1.
SPIN_DEV = (8.63e-7, 8.63e-7, 2.89e-3)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_torque_free_spin(axis):
    """A dry body spinning at 3 rad/s about a principal axis: after n steps of the Cayley map it has turned by
    n * 2 atan(h w / 2) about that axis, and R stays orthonormal within the derived bound at every step."""
    n, w = 1000, 3.0
    props = S.props(100.0, (10.0, 20.0, 30.0))[None]
    spin = [0.0, 0.0, 0.0]
    spin[axis] = w
    p32 = H.pose(c=(0.0, 500.0, 0.0), w=spin)[None]
    p64 = p32.astype(np.float64)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    step_angle = 2.0 * np.arctan(float(F(DT)) * w / 2.0)

    def wrapped(x):
        return (x + np.pi) % (2.0 * np.pi) - np.pi

    dev = err = ortho = 0.0
    for k in range(1, n + 1):
        p32, _, _ = S.hull_step(S.dry_loads, p32, props, DT, 1, gravity=(0.0, 0.0, 0.0))
        p64, _, _ = S.hull_step(S.dry_loads, p64, props, DT, 1, gravity=(0.0, 0.0, 0.0), dtype=np.float64)
        a32 = np.arctan2(float(p32[0, 3 * j + i]), float(p32[0, 3 * i + i]))
        a64 = np.arctan2(p64[0, 3 * j + i], p64[0, 3 * i + i])
        assert abs(wrapped(a64 - k * step_angle)) < 1e-10
        dev, err = max(dev, abs(wrapped(a32 - a64))), max(err, abs(wrapped(a32 - k * step_angle)))
        ortho = max(ortho, _ortho_error(p32))
    print(f"spin about axis {axis}: float32 - float64 angle at most {dev:.3e} rad, against n * 2 atan(h w / 2) "
          f"{err:.3e} (gate {4 * SPIN_DEV[axis]:.3e}); |R R^T - I| at most {ortho:.3e} (bound {ORTHO_BOUND:.3e})")
    assert err <= 4 * SPIN_DEV[axis]
    assert ortho <= ORTHO_BOUND
    # the axis is fixed, the centre does not move
    assert p32[0, 3 * axis + axis] == pytest.approx(1.0, abs=ORTHO_BOUND) and np.array_equal(p32[0, 9:15], [0, 500, 0, 0, 0, 0])


FLOAT_STEPS = 600  # chosen on the CPU: from step 500 on the restatement's imbalance is 8.8e-4 N, the gate 3.7e-2 N


def test_flat_water_float(oracle):
    """box_hull() with the mass of half its displaced volume, released 0.3 m high and rolled 0.2 rad over flat
    water, damping 4 / s: after FLOAT_STEPS steps it floats. |F.y + mass g.y| is within the loads' own sum bound
    (FOLD_BOUND * sum|a_i|, test_hulls.py) times 1: the body has come to rest, so what is left is the
    rounding of the sum it rests on. The roll has decayed."""
    cas = _oracle_scene(oracle, 64, scale=0.0)
    hull = H.box_hull()
    ranges = np.array([[0, 64]], np.int32)
    mass = 0.5 * float(hull[:, 3].astype(np.float64).sum()) * RHO_G / 9.8  # equilibrium draft: half the box
    props = S.props(mass, S.box_inertia(mass, (2.0, 1.0, 4.0)), 4.0, 4.0)[None]
    poses = H.pose(_rot_z(0.2), c=(3.0, 0.3, -7.0))[None]
    loads_fn = S.water_loads(oracle, cas, None, hull, ranges, RHO_G, 8, 0.0, False)
    for _ in range(FLOAT_STEPS):
        poses, _, _ = S.hull_step(loads_fn, poses, props, DT, 1)
    loads, _, info = H.hull_loads(oracle, cas, None, hull, ranges, poses, RHO_G, 8, 0.0, False)
    bound = 1.0 * FOLD_BOUND * float(np.abs(info["a"][:, 1].astype(np.float64)).sum())
    imbalance = abs(float(loads[0, 1]) + float(F(mass)) * float(F(-9.8)))
    roll = float(np.arctan2(poses[0, 3], poses[0, 0]))
    print(f"flat-water float after {FLOAT_STEPS} steps: imbalance {imbalance:.3e} N (gate {bound:.3e}), roll {roll:.3e} rad, "
          f"c.y {poses[0, 10]:.3e}, submerged volume {loads[0, 3]} of {hull[:, 3].sum()}")
    assert imbalance <= bound
    assert abs(roll) < 0.2 and abs(roll) < 1e-3
    assert abs(float(poses[0, 10])) < 1e-3 and _ortho_error(poses) <= ORTHO_BOUND


def test_kinematic_body_keeps_its_velocities(oracle):
    """kinematic = 1 under full wave loads: v and w keep their bits and c advances by h v every substep."""
    cas = _oracle_scene(oracle, 64)
    rng = np.random.default_rng(5)
    points = _random_points(rng, 40)
    ranges = np.array([[0, 40], [3, 20]], np.int32)
    start = _random_poses(rng, 2)
    props = np.stack([S.props(50.0, (5.0, 6.0, 7.0), 1.0, 1.0, 1.0)] * 2)
    loads_fn = S.water_loads(oracle, cas, None, points, ranges, RHO_G, 8, 0.0, False)
    poses, loads, _ = S.hull_step(loads_fn, start, props, DT, 3)
    assert np.any(loads[:, :3] != 0.0)  # the water does push
    assert poses[:, 12:18].tobytes() == start[:, 12:18].tobytes()
    h = F(DT) / F(3)
    c = start[:, 9:12]
    for _ in range(3):
        c = c + h * start[:, 12:15]
    assert c.dtype == F and np.array_equal(poses[:, 9:12], c)
    assert not np.array_equal(poses[:, :9], start[:, :9]) and _ortho_error(poses) <= ORTHO_BOUND
    free, _, _ = S.hull_step(loads_fn, start, np.stack([S.props(50.0, (5.0, 6.0, 7.0), 1.0, 1.0, 0.0)] * 2), DT, 3)
    assert not np.array_equal(free[:, 12:18], start[:, 12:18])


def test_null_and_zero_wrench_agree(oracle):
    """wrench_ext null and all zero: equal poses (adding +0 changes no value)."""
    cas = _oracle_scene(oracle, 64)
    rng = np.random.default_rng(6)
    points = _random_points(rng, 33)
    ranges = np.array([[0, 33], [5, 16], [0, 1]], np.int32)
    start = _random_poses(rng, 3)
    props = np.stack([S.props(60.0, (5.0, 6.0, 7.0), 0.5, 0.25)] * 3)
    loads_fn = S.water_loads(oracle, cas, None, points, ranges, RHO_G, 8, 0.0, False)
    none, _, _ = S.hull_step(loads_fn, start, props, DT, 2)
    zero, _, _ = S.hull_step(loads_fn, start, props, DT, 2, ext=np.zeros((3, 8), F))
    assert np.array_equal(none, zero) and not np.array_equal(none, start)
    push = np.zeros((3, 8), F)
    push[1, 0], push[2, 5] = 500.0, 40.0
    pushed, _, _ = S.hull_step(loads_fn, start, props, DT, 2, ext=push)
    assert np.array_equal(pushed[0], none[0]) and pushed[1, 12] > none[1, 12] and not np.array_equal(pushed[2], none[2])


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


@pytest.fixture(scope="module")
def calm64(ocean):
    return _scene(ocean, 64)


@pytest.fixture(scope="module")
def steep64(ocean):
    return _scene(ocean, 64, **STEEP)


def _hull_set(sampler, points, ranges, props=None):
    from oceansimulation_amd.surface import HullSet

    hulls = HullSet(sampler.fft, points, ranges)
    if props is not None:
        hulls.set_bodies(props)
    return hulls


def _random_props(rng, points, ranges, kinematic=None):
    """Bodies that float: about half their displaced volume of water as mass, moments of that order."""
    out = np.zeros((len(ranges), 8), F)
    for b, (first, count) in enumerate(ranges):
        mass = rng.uniform(0.3, 0.8) * 1000.0 * float(points[first:first + count, 3].sum())
        out[b] = S.props(mass, mass * rng.uniform(0.5, 3.0, 3), rng.uniform(0.0, 2.0), rng.uniform(0.0, 2.0),
                         0.0 if kinematic is None else kinematic[b])
    return out


def _reference_calls(oracle, scene, points, ranges, poses, props, calls, substeps, velocity, iterations=8, tolerance=0.0,
                     ext=None, gravity=S.GRAVITY, dt=DT):
    """[(poses, loads, point_out)] after each of `calls` successive ocean_hulls_step calls, restated."""
    _, host, rates = scene
    loads_fn = S.water_loads(oracle, host, rates if velocity else None, points, ranges, RHO_G, iterations, tolerance,
                             velocity)
    out = []
    for _ in range(calls):
        poses, loads, pts = S.hull_step(loads_fn, poses, props, dt, substeps, gravity, ext)
        out.append((poses, loads, pts))
    return out


def _check_calls(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert not np.isnan(w[0]).any(), (what, "call", k, "the reference has NaN poses")
        for name, a, b in zip(("poses", "loads", "point_out"), g, w):
            assert np.array_equal(a, b), (what, "call", k, name, float(np.max(np.abs(a - b))))
        assert np.all(g[0][:, 18:] == 0.0)


SMALL_COUNTS = (1, 5, 16, 33, 64)


def _small_bodies(seed=64):
    """Bodies of every count in SMALL_COUNTS on shared ranges of one 64-point hull, in runs that pack (four
    16-point bodies and twelve 5-point bodies to a wave, 64 one-point bodies and a partly filled wave of them),
    runs broken by other sizes, and full waves: every body is one tile, so a call is one launch."""
    rng = np.random.default_rng(seed)
    points = _random_points(rng, 64)
    counts = [16] * 5 + [5] * 11 + [64] + [1] * 70 + [33, 33] + [16, 5, 1, 64, 33] + [5] * 3
    ranges = np.array([(int(rng.integers(0, 64 - n + 1)), n) for n in counts], np.int32)
    assert set(counts) == set(SMALL_COUNTS) and max(counts) <= 64
    return points, ranges, _random_poses(rng, len(counts)), _random_props(rng, points, ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("velocity", [False, True])
@pytest.mark.parametrize("scene_name", ["calm", "steep"])
def test_small_bodies_bit_exact(ocean, oracle, calm64, steep64, scene_name, velocity, substeps):
    """Point counts 1, 5, 16, 33 and 64 (packed segments, a full wave; the one-launch path): one call, and then 8
    successive calls on the device's own poses, each compared with the restatement: poses, loads, point_out."""
    scene = calm64 if scene_name == "calm" else steep64
    iterations, tolerance = (8, 0.0) if scene_name == "calm" else (16, 1e-4)
    points, ranges, poses, props = _small_bodies()
    hulls = _hull_set(scene[0], points, ranges, props)
    kw = dict(dt=DT, substeps=substeps, iterations=iterations, tolerance=tolerance, water_velocity=int(velocity), rho_g=RHO_G)
    want = _reference_calls(oracle, scene, points, ranges, poses, props, 9, substeps, velocity, iterations, tolerance)
    _check_calls(hulls.step_host(scene[0], poses, calls=1, **kw), want[:1], "one call")
    _check_calls(hulls.step_host(scene[0], poses, calls=9, **kw)[1:], want[1:], "successive calls")
    s = want[-1][2][:, 7]
    assert (s > 0).any() and not np.array_equal(want[-1][0], want[0][0])
    assert _ortho_error(want[-1][0]) <= ORTHO_BOUND
    hulls.close()


def _mixed_bodies(seed=4097):
    """One-tile bodies (alone and packed) among bodies of 65, 257 and 4097 points: integration in the fold kernel
    after a two- and a three-level fold, and both kinds of body in one call."""
    rng = np.random.default_rng(seed)
    points = _random_points(rng, 4097)
    counts = [16, 16, 65, 5, 257, 64, 4097, 1, 1, 1, 33, 65]
    ranges = np.array([(int(rng.integers(0, 4097 - n + 1)), n) for n in counts], np.int32)
    return points, ranges, _random_poses(rng, len(counts)), _random_props(rng, points, ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 3])
def test_bodies_of_several_tiles_bit_exact(ocean, oracle, calm64, substeps):
    points, ranges, poses, props = _mixed_bodies()
    hulls = _hull_set(calm64[0], points, ranges, props)
    kw = dict(dt=DT, substeps=substeps, water_velocity=1, rho_g=RHO_G)
    want = _reference_calls(oracle, calm64, points, ranges, poses, props, 3, substeps, True)
    _check_calls(hulls.step_host(calm64[0], poses, calls=3, **kw), want, f"mixed set, {substeps} substeps")
    assert np.all(want[-1][1][ranges[:, 1] > 64, 7] > 0)  # the bodies of several tiles are in the water
    hulls.close()


@pytest.mark.gpu
def test_packed_and_unpacked_sets_agree(ocean, calm64):
    """ocean_debug_hulls_packing(0): every body on its own wave; equal poses, loads and rows."""
    from oceansimulation_amd import capi

    sampler = calm64[0]
    points, ranges, poses, props = _small_bodies(seed=65)
    kw = dict(dt=DT, substeps=3, water_velocity=1, rho_g=RHO_G)
    packed = _hull_set(sampler, points, ranges, props).step_host(sampler, poses, calls=2, **kw)
    capi.lib().ocean_debug_hulls_packing(0)
    try:
        own = _hull_set(sampler, points, ranges, props)
    finally:
        capi.lib().ocean_debug_hulls_packing(1)
    _check_calls(own.step_host(sampler, poses, calls=2, **kw), packed, "own waves against packed")


@pytest.mark.gpu
def test_instances_in_one_call_and_alone(ocean, calm64):
    """One 16-point hull at 300 poses in one call (four bodies to a wave) equals 300 one-body calls."""
    sampler = calm64[0]
    rng = np.random.default_rng(300)
    points = _random_points(rng, 16)
    poses = _random_poses(rng, 300)
    ranges = np.tile(np.array([[0, 16]], np.int32), (300, 1))
    props = _random_props(rng, points, ranges)
    kw = dict(dt=DT, substeps=2, water_velocity=1, rho_g=RHO_G)
    many = _hull_set(sampler, points, ranges, props).step_host(sampler, poses, **kw)[0]
    one = _hull_set(sampler, points, ranges[:1])
    for b in range(300):
        one.set_bodies(props[b:b + 1])  # replaces the properties
        pb, lb, rb = one.step_host(sampler, poses[b], **kw)[0]
        assert pb.tobytes() == many[0][b:b + 1].tobytes() and lb.tobytes() == many[1][b:b + 1].tobytes(), b
        assert rb.tobytes() == many[2][16 * b:16 * b + 16].tobytes(), b


@pytest.mark.gpu
@pytest.mark.parametrize("bodies", ["small", "mixed"])
def test_replay_and_in_place(ocean, calm64, bodies):
    """The same call twice from the same start is byte-identical; and stepping a buffer in place gives what the
    step of a device copy of it gives (only the owner of a body writes its pose, after every read of it)."""
    from oceansimulation_amd.hip import DeviceBuffer

    sampler = calm64[0]
    points, ranges, poses, props = _small_bodies(7) if bodies == "small" else _mixed_bodies(8)
    hulls = _hull_set(sampler, points, ranges, props)
    kw = dict(dt=DT, substeps=4, water_velocity=1, rho_g=RHO_G)
    first = hulls.step_host(sampler, poses, calls=2, **kw)
    again = hulls.step_host(sampler, poses, calls=2, **kw)
    for a, b in zip(first, again):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    src = DeviceBuffer.from_array(poses)
    copy = DeviceBuffer.from_array(src.to_host(poses.shape))
    hulls.step(sampler, src.ptr, **kw)
    hulls.step(sampler, copy.ptr, **kw)
    hulls.fft.synchronize()
    assert src.to_host(poses.shape).tobytes() == copy.to_host(poses.shape).tobytes() == first[0][0].tobytes()


# One wave (64 threads) per tile in k_hulls_step, 256 threads per body of several tiles in k_hulls_step_fold. A
# workgroup of WG threads is resident at most min(32, 2048 / WG) times per CU (32 workgroup slots, 2048 threads),
# so at budget 1 the grid has at most 32 (8) workgroups, and with items >= 3 * 32 (folds >= 3 * 8) some
# workgroup runs three or more items (tests/test_item_loops.py states the same rule for the loads).
@pytest.mark.gpu
@pytest.mark.parametrize("case", [dict(id="1024x16", bodies=1024, points=16, folds=0),
                                  dict(id="100x70", bodies=100, points=70, folds=100)], ids=lambda c: c["id"])
def test_budgeted_step_equals_full_device(ocean, calm64, case):
    sampler = calm64[0]
    fft = sampler.fft
    rng = np.random.default_rng(case["bodies"])
    points = _random_points(rng, case["points"])
    ranges = np.tile(np.array([[0, case["points"]]], np.int32), (case["bodies"], 1))
    poses = _random_poses(rng, case["bodies"])
    hulls = _hull_set(sampler, points, ranges, _random_props(rng, points, ranges))
    tiles = case["bodies"] // 4 if case["points"] == 16 else case["bodies"] * 2  # four 16-point bodies to a wave
    assert tiles >= 3 * 1 * min(32, 2048 // 64) and (case["folds"] == 0 or case["folds"] >= 3 * 1 * min(32, 2048 // 256))
    kw = dict(dt=DT, substeps=3, water_velocity=1, rho_g=RHO_G)
    try:
        full = hulls.step_host(sampler, poses, calls=2, **kw)
        fft.set_cu_budget(1)
        one = hulls.step_host(sampler, poses, calls=2, **kw)
    finally:
        fft.set_cu_budget(0)
    _check_calls(one, full, "budget 1 against the full device")
    hulls.close()


@pytest.mark.gpu
def test_kinematic_dynamic_and_wrenches(ocean, oracle, calm64):
    """Kinematic and dynamic bodies in one set, and wrench_ext on some bodies (null, zero rows, forces and
    torques), against the restatement; a kinematic body keeps the bits of its velocities."""
    rng = np.random.default_rng(11)
    points, ranges, poses, _ = _mixed_bodies(12)
    kinematic = (np.arange(len(ranges)) % 3 == 0).astype(F)
    props = _random_props(rng, points, ranges, kinematic)
    ext = np.zeros((len(ranges), 8), F)
    ext[1::2, :3] = rng.uniform(-200.0, 200.0, (len(ext[1::2]), 3))
    ext[1::2, 4:7] = rng.uniform(-50.0, 50.0, (len(ext[1::2]), 3))
    ext[:, 3], ext[:, 7] = 7.0, -3.0  # not read
    hulls = _hull_set(calm64[0], points, ranges, props)
    kw = dict(dt=DT, substeps=2, water_velocity=1, rho_g=RHO_G, gravity=(0.5, -9.8, -0.25))
    want = _reference_calls(oracle, calm64, points, ranges, poses, props, 2, 2, True, ext=ext, gravity=(0.5, -9.8, -0.25))
    got = hulls.step_host(calm64[0], poses, ext=ext, calls=2, **kw)
    _check_calls(got, want, "kinematic and dynamic bodies with wrenches")
    k = kinematic != 0
    assert got[-1][0][k, 12:18].tobytes() == poses[k, 12:18].tobytes()
    assert not np.array_equal(got[-1][0][~k, 12:18], poses[~k, 12:18])
    none = hulls.step_host(calm64[0], poses, calls=1, **kw)
    zero = hulls.step_host(calm64[0], poses, ext=np.zeros_like(ext), calls=1, **kw)
    _check_calls(zero, none, "zero wrenches against null")
    assert not np.array_equal(none[0][0], got[0][0])


@pytest.mark.gpu
def test_invalid_step_calls_fail_loudly(ocean):
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.hip import DeviceBuffer
    from oceansimulation_amd.surface import HullSet, SurfaceSampler

    fft = ocean.FFTCalculator(64)
    gens = [ocean.Generator(fft, 1) for _ in range(2)]
    for g in gens:
        g.CalculateOcean(1.0)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    hulls = HullSet(fft, H.box_hull(), np.array([[0, 64], [0, 64]], np.int32))
    poses = np.stack([H.pose(), H.pose(c=(5.0, 0.0, 5.0))])
    good = np.stack([S.props(100.0, (10.0, 20.0, 30.0), 0.5, 0.5)] * 2)
    with pytest.raises(OceanError, match="ocean_hulls_step: the bodies' properties were never set"):
        hulls.step_host(sampler, poses)

    def bad(slot, value):
        p = good.copy()
        p[1, slot] = value
        return p

    for name, p in {"nan mass": bad(0, np.nan), "zero mass": bad(0, 0.0), "negative moment": bad(2, -1.0),
                    "infinite moment": bad(3, np.inf), "negative linear damping": bad(4, -0.1),
                    "negative angular damping": bad(5, -0.1), "kinematic 2": bad(6, 2.0), "kinematic 0.5": bad(6, 0.5),
                    "nan padding": bad(7, np.nan)}.items():
        with pytest.raises(OceanError, match="ocean_hulls_set_bodies: body 1"):
            hulls.set_bodies(p)
    with pytest.raises(OceanError, match="never set"):  # a refused set_bodies sets nothing
        hulls.step_host(sampler, poses)
    hulls.set_bodies(good)
    assert hulls.step_host(sampler, poses)[0][0].shape == (2, 20)
    for kw in (dict(dt=0.0), dict(dt=float("nan")), dict(substeps=0), dict(substeps=65), dict(gravity=(0.0, float("inf"), 0.0)),
               dict(iterations=-1), dict(iterations=65), dict(tolerance=-1.0), dict(rho_g=float("inf")),
               dict(water_velocity=2)):
        with pytest.raises(OceanError, match="ocean_hulls_step"):
            hulls.step_host(sampler, poses, **kw)
    gens[0].calculate_rates()
    with pytest.raises(OceanError, match="ocean_hulls_step: generator 1 has no rates"):
        hulls.step_host(sampler, poses, water_velocity=1)
    gens[1].calculate_rates()
    assert hulls.step_host(sampler, poses, water_velocity=1, substeps=64)[0][0].shape == (2, 20)
    foreign = ocean.Generator(ocean.FFTCalculator(64), 1)
    foreign.CalculateOcean(1.0)
    with pytest.raises(OceanError, match="ocean_hulls_step: the first generator is on another plan than the hull set"):
        hulls.step_host(SurfaceSampler([(foreign, 0)]), poses)
    with pytest.raises(OceanError, match="null settings/poses"):
        hulls.step(sampler, 0)
    buf = DeviceBuffer.from_array(poses)
    hulls.step(sampler, buf.ptr)  # no loads, no point_out, no wrenches
    fft.synchronize()
    assert np.array_equal(buf.to_host(poses.shape), hulls.step_host(sampler, poses)[0][0])


@pytest.mark.gpu
def test_existing_calls_after_a_step(ocean, oracle, calm64):
    """ocean_hulls_loads on the same set and a surface query after steps on both paths: their usual bits."""
    sampler, host, rates = calm64
    rng = np.random.default_rng(13)
    xz = rng.uniform(-400.0, 400.0, (3000, 2)).astype(F)
    want_q = surface_query(oracle, host, xz, 4, 0.0)
    for points, ranges, poses, props in (_small_bodies(14), _mixed_bodies(15)):
        hulls = _hull_set(sampler, points, ranges, props)
        stepped = hulls.step_host(sampler, poses, dt=DT, substeps=2, water_velocity=1, rho_g=RHO_G)[0][0]
        loads, pts = hulls.loads_host(sampler, stepped, RHO_G, 8, 0.0, True)
        want_loads, want_pts, _ = H.hull_loads(oracle, host, rates, points, ranges, stepped, RHO_G, 8, 0.0, True)
        assert np.array_equal(loads, want_loads) and np.array_equal(pts, want_pts)
        assert np.array_equal(sampler.query_host(xz.copy(), 4, 0.0), want_q)
        hulls.close()


@pytest.mark.gpu
def test_waveapp_headless_float_bodies(ocean, oracle, tmp_path):
    """--float-bodies: the released bodies' poses in the JSON line equal the restatement stepped once from the
    dumped start poses on the maps and rate maps the example dumped."""
    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "1", "--mesh", "0", "--bodies", "16", "--float-bodies", "--dump",
                        str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    scene = json.load(open(tmp_path / "scene.json"))
    cas = [(np.load(tmp_path / f"height_{i}.npy"), np.load(tmp_path / f"disp_{i}.npy"), np.load(tmp_path / f"jac_{i}.npy"),
            c["planeSize"], c["displacement"]) for i, c in enumerate(scene["cascades"])]
    rates = [(np.load(tmp_path / f"height_rate_{i}.npy"), np.load(tmp_path / f"disp_rate_{i}.npy")) for i in range(3)]
    points, ranges = np.load(tmp_path / "hull_points.npy"), np.load(tmp_path / "hull_ranges.npy")
    start, props = np.load(tmp_path / "body_poses.npy"), np.load(tmp_path / "body_props.npy")
    assert start.shape == (16, 20) and props.shape == (16, 8) and np.all(props[:, 6] == 0.0)
    assert props[0, 0] == F(0.5) * F(8.0) * (F(scene["bodies"]["rho_g"]) / F(9.8))
    b = scene["bodies"]
    loads_fn = S.water_loads(oracle, cas, rates, points, ranges, b["rho_g"], 8, 0.0, True)
    want, want_loads, want_pts = S.hull_step(loads_fn, start, props, b["dt"], b["substeps"], b["gravity"])
    got = np.array(out["body_poses"], F)
    assert got.shape == (16, 20) and np.array_equal(got, want)
    assert np.array_equal(np.load(tmp_path / "body_poses_final.npy"), want)
    assert np.array_equal(np.load(tmp_path / "body_loads.npy"), want_loads)
    assert np.array_equal(np.load(tmp_path / "body_points.npy"), want_pts)
    assert b["substeps"] == 2 and not np.array_equal(want[:, 9:12], start[:, 9:12])
