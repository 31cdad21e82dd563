"""ocean_moorings: mooring lines stepped on the device and the wrenches they put on hull bodies, against the
contract restated in numpy float32 (tests/moorings_ref.py on tests/kinematics_ref.py and tests/hull_loads_ref.py).

The CPU tests pin the restatement itself on closed forms (a slack line, a taut line, the vertical balance of a
hanging line, a node resting on the bed) and the host's argument checks. The GPU tests compare the kernels with
the restatement on the GPU's own maps with np.array_equal: nodes, line_out and wrench_ext, bit for bit. Scenes
as in test_hulls.py (N = 64, three cascades; "calm" the defaults, "steep" displacement = 1 and scale = 2), with
the depth layers (0, 0.5, 2, 8) m.

Gates of the closed-form tests, by the rule of test_hull_step.py: the closed forms are those of the recurrence
itself at rest, so a float64 evaluation of the same recurrence on the same float32 inputs agrees with them far
below float32's resolution (asserted); what the float32 restatement adds is its rounding. That deviation was
measured once with moorings_ref's dtype=float64 over the inputs of each test, is written at the test, and the
test gates at 4 times it. Nothing here is measured against the device code.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hull_loads_ref as H
import hull_step_ref as S
import kinematics_ref as K
import moorings_ref as M
from test_hulls import RHO_G, STEEP, _random_points, _random_poses, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DT = 1.0 / 60.0
DEPTHS = (0.0, 0.5, 2.0, 8.0)
NODE_COUNTS = (2, 3, 5, 31, 32, 33, 64, 4, 4, 7, 64, 2)
NEW_CALLS = ("ocean_moorings_create", "ocean_moorings_destroy", "ocean_moorings_lines", "ocean_moorings_total_nodes",
             "ocean_moorings_nodes", "ocean_moorings_reset", "ocean_default_mooring_settings", "ocean_moorings_step")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- without a GPU ----------------------------------------------------------------------------
def _create(L, lines, attach, n_lines, bodies, fft=True, out=True):
    """ocean_moorings_create with a stand-in for the plan (the argument checks come before any use of it)."""
    h = ctypes.c_void_p()
    plan = ctypes.create_string_buffer(4096)
    rc = L.ocean_moorings_create(ctypes.byref(h) if out else None, ctypes.addressof(plan) if fft else None,
                                 None if lines is None else lines.ctypes.data,
                                 None if attach is None else attach.ctypes.data, n_lines, bodies)
    assert not h.value
    return rc, L.ocean_last_error()


def test_moorings_are_exported_and_reject_bad_arguments():
    from oceansimulation_amd import capi
    from oceansimulation_amd.surface import MooringSet

    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    for name in ("reset", "step", "step_host", "nodes_host", "settings", "close"):
        assert hasattr(MooringSet, name), name
    d = MooringSet.settings()
    assert (d.substeps, d.iterations, d.water) == (8, 4, 0) and d.dt == F(DT) and d.tolerance == 0.0
    assert list(d.gravity) == [0.0, F(-9.8), 0.0] and d.rho_g == 9810.0
    assert (d.bed_y, d.bed_k, d.bed_c) == (-100.0, F(1e5), F(1e3))
    L.ocean_default_mooring_settings(None)  # a null pointer is ignored
    with pytest.raises(AttributeError):
        MooringSet.settings(depth=1.0)

    good = np.stack([M.line((0, -10, 0), (1, 0, 0), 12.0, 1e5, 10.0, 5.0, 1e-3, 1.0, 2.0)] * 2)
    att = np.array([[0, 8], [-1, 2]], np.int32)

    def bad(slot, value):
        x = good.copy()
        x[1, slot] = value
        return x

    def bad_att(col, value):
        a = att.copy()
        a[1, col] = value
        return a

    cases = {
        "null out": (dict(out=False), b"null argument"),
        "null fft": (dict(fft=False), b"null argument"),
        "null lines": (dict(lines=None), b"null argument"),
        "null attach": (dict(attach=None), b"null argument"),
        "no lines": (dict(n_lines=0), b"n_lines outside 1..1048576"),
        "too many lines": (dict(n_lines=1048577), b"n_lines outside 1..1048576"),
        "negative bodies": (dict(bodies=-1), b"bodies outside 0..1048576"),
        "too many bodies": (dict(bodies=1048577), b"bodies outside 0..1048576"),
        "body -2": (dict(attach=bad_att(0, -2)), b"line 1 has a body outside"),
        "body == bodies": (dict(attach=bad_att(0, 1)), b"line 1 has a body outside"),
        "one node": (dict(attach=bad_att(1, 1)), b"line 1 has a node count outside 2..64"),
        "65 nodes": (dict(attach=bad_att(1, 65)), b"line 1 has a node count outside 2..64"),
        "nan anchor": (dict(lines=bad(1, np.nan)), b"line 1 has a non-finite field"),
        "inf padding": (dict(lines=bad(15, np.inf)), b"line 1 has a non-finite field"),
        "zero length": (dict(lines=bad(6, 0.0)), b"length, EA and mass_per_m > 0"),
        "negative EA": (dict(lines=bad(7, -1.0)), b"length, EA and mass_per_m > 0"),
        "zero mass": (dict(lines=bad(9, 0.0)), b"length, EA and mass_per_m > 0"),
        "negative CA": (dict(lines=bad(8, -1.0)), b"CA, volume_per_m and drag coefficients >= 0"),
        "negative volume": (dict(lines=bad(10, -1e-3)), b"CA, volume_per_m and drag coefficients >= 0"),
        "negative drag_lin": (dict(lines=bad(11, -1.0)), b"CA, volume_per_m and drag coefficients >= 0"),
        "negative drag_quad": (dict(lines=bad(12, -1.0)), b"CA, volume_per_m and drag coefficients >= 0"),
        "padding set": (dict(lines=bad(14, 1.0)), b"slots 13..15 zero"),
    }
    for name, (kw, message) in cases.items():
        args = dict(lines=good, attach=att, n_lines=2, bodies=1)
        args.update(kw)
        rc, err = _create(L, **args)
        assert rc == capi.OCEAN_ERR_INVALID and b"ocean_moorings_create" in err and message in err, (name, rc, err)

    assert L.ocean_moorings_lines(None) == 0 and L.ocean_moorings_total_nodes(None) == 0
    assert not L.ocean_moorings_nodes(None) and L.ocean_moorings_destroy(None) == capi.OCEAN_OK
    assert L.ocean_moorings_reset(None, None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_moorings_reset: null mooring set" in L.ocean_last_error()

    stand_in = ctypes.create_string_buffer(4096)  # a set with no line on a body, no bodies, never reset
    moorings = ctypes.addressof(stand_in)

    def step(m=moorings, settings=d):
        rc = L.ocean_moorings_step(m, None, None, 0, ctypes.byref(settings) if settings is not None else None, None,
                                   None, None)
        return rc, L.ocean_last_error()

    nan, inf = float("nan"), float("inf")
    s = MooringSet.settings
    cases = {
        "null set": (dict(m=None), b"null mooring set"),
        "null settings": (dict(settings=None), b"null settings"),
        "dt 0": (dict(settings=s(dt=0.0)), b"dt must be finite and > 0"),
        "dt negative": (dict(settings=s(dt=-DT)), b"dt must be finite and > 0"),
        "dt nan": (dict(settings=s(dt=nan)), b"dt must be finite and > 0"),
        "dt inf": (dict(settings=s(dt=inf)), b"dt must be finite and > 0"),
        "substeps 0": (dict(settings=s(substeps=0)), b"substeps outside 1..256"),
        "substeps 257": (dict(settings=s(substeps=257)), b"substeps outside 1..256"),
        "gravity nan": (dict(settings=s(gravity=(0.0, nan, 0.0))), b"gravity must be finite"),
        "gravity inf": (dict(settings=s(gravity=(inf, 0.0, 0.0))), b"gravity must be finite"),
        "rho_g negative": (dict(settings=s(rho_g=-1.0)), b"rho_g must be finite and >= 0"),
        "rho_g inf": (dict(settings=s(rho_g=inf)), b"rho_g must be finite and >= 0"),
        "iterations 65": (dict(settings=s(iterations=65)), b"iterations outside 0..64"),
        "tolerance nan": (dict(settings=s(tolerance=nan)), b"tolerance must be finite"),
        "water 2": (dict(settings=s(water=2)), b"water must be 0 or 1"),
        "bed_y nan": (dict(settings=s(bed_y=nan)), b"bed_y must be finite"),
        "bed_k negative": (dict(settings=s(bed_k=-1.0)), b"bed_k and bed_c must be finite and >= 0"),
        "bed_c inf": (dict(settings=s(bed_c=inf)), b"bed_k and bed_c must be finite and >= 0"),
        "never reset": (dict(), b"the nodes were never reset nor written"),
        "water without generators": (dict(settings=s(water=1, substeps=256)), b"never reset"),
    }
    for name, (kw, message) in cases.items():
        rc, err = step(**kw)
        assert rc == capi.OCEAN_ERR_INVALID and b"ocean_moorings_step" in err and message in err, (name, rc, err)


def test_cpp_header_compiles_standalone(tmp_path):
    """A consumer of the mooring lines compiles against the drop-in headers alone."""
    src = tmp_path / "consumer.cpp"
    src.write_text(
        '#include "waves/Surface.h"\n'
        "#include <vector>\n"
        "void frame(Waves::MooringSet& m, Waves::HullSet& h, std::vector<Waves::Generator*>& gens, float* poses) {\n"
        "  ocean_mooring_settings ms; ocean_default_mooring_settings(&ms); ms.water = 1;\n"
        "  ocean_hull_step_settings hs; ocean_default_hull_step_settings(&hs);\n"
        "  for (auto* g : gens) { g->CalculateOcean(hs.dt); g->CalculateRates(); g->CalculateKinematics(); }\n"
        "  m.Step(gens, ms, poses, true);\n"
        "  h.Step(gens, poses, hs, m.GetWrenchDevice());\n"
        "  Vision::ID rows = m.GetLineOutput(); (void)rows;\n"
        "  if (m.GetLines() < 1 || m.GetTotalNodes() < 2 || !m.GetNodesDevice() || !m.GetHandle()) m.Reset(poses);\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}/include", "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    so = os.path.join(ROOT, "oceansimulation_amd", "libwaves.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", so], capture_output=True, text=True).stdout
    for sig in ("Waves::MooringSet::MooringSet(", "Waves::MooringSet::Reset(float const*)", "Waves::MooringSet::Step(",
                "Waves::MooringSet::GetWrenchDevice() const"):
        assert sig in syms, sig


def test_slack_line_stays_at_rest():
    """Zero gravity, ends 6 m apart on a 9 m line of 7 nodes, at rest: every T is 0 and no node moves, by exact
    equality, over 10 calls of 8 substeps."""
    lines = M.line((1.0, -3.0, 2.0), (5.0, -1.0, 6.0), 9.0, 1e6, 50.0, 4.0, 0.0, 3.0, 2.0)[None]
    attach = np.array([[-1, 7]], np.int32)
    start = M.reset(lines, attach)
    assert np.linalg.norm(lines[0, 3:6] - lines[0, 0:3]) == 6.0
    nodes = start
    for _ in range(10):
        nodes, out, wrench = M.mooring_step(lines, attach, nodes, None, 0, gravity=(0.0, 0.0, 0.0))
        assert nodes.dtype == F and np.array_equal(nodes[:, :3], start[:, :3]) and np.all(nodes[:, 3:7] == 0.0)
        assert np.all(out[0, :6] == 0.0) and out[0, 7] == 5.0 and out[0, 6] == 0.0 and wrench.shape == (0, 8)
    assert np.array_equal(nodes[:, 7], [0, 1, 1, 1, 1, 1, 0])  # the interior nodes are wet, the ends carry no flag


# the largest |float32 - float64| of the restatement over test_taut_line's inputs, measured once: the tensions
# (N, of 2.4e4 N) and the components of Fm
TAUT_DEV_T, TAUT_DEV_F = 6.01e-5, 3.95e-4


def test_taut_line_carries_the_strain():
    """Zero gravity, two fixed ends D = 13 m apart on a slanted axis, a 12.4 m line of 9 evenly spaced nodes: every
    segment carries EA (D / (n - 1) - l0) / l0, and Fm is that tension from the fairlead towards the anchor."""
    n, ea, length = 9, 5e5, 12.4
    A, B = np.array([2.0, -9.0, 1.0]), np.array([5.0, 3.0, 5.0])
    D = float(np.linalg.norm(B - A))
    assert D == 13.0
    lines = M.line(A, B, length, ea, 0.0, 4.0)[None]
    attach = np.array([[-1, n]], np.int32)
    start = M.reset(lines, attach)
    kw = dict(substeps=1, gravity=(0.0, 0.0, 0.0))
    n32, o32, _ = M.mooring_step(lines, attach, start, None, 0, **kw)
    n64, o64, _ = M.mooring_step(lines, attach, start, None, 0, dtype=np.float64, **kw)
    l0 = float(F(length) / F(n - 1))
    want_t = float(F(ea)) * (D / (n - 1) - l0) / l0
    want_f = -want_t * (B - A) / D
    assert np.abs(n64[:-1, 3] - want_t).max() < 1e-6 * want_t and np.abs(o64[0, :3] - want_f).max() < 1e-6 * want_t
    dev_t = float(np.abs(n32[:-1, 3].astype(np.float64) - n64[:-1, 3]).max())
    dev_f = float(np.abs(o32[0, :3].astype(np.float64) - o64[0, :3]).max())
    err_t = float(np.abs(n32[:-1, 3].astype(np.float64) - want_t).max())
    err_f = float(np.abs(o32[0, :3].astype(np.float64) - want_f).max())
    print(f"taut line: T = {want_t:.6e} N; float32 - float64 at most {dev_t:.3e} N (T), {dev_f:.3e} N (Fm); against the "
          f"closed form {err_t:.3e}, {err_f:.3e}; gates {4 * TAUT_DEV_T:.3e}, {4 * TAUT_DEV_F:.3e}")
    assert err_t <= 4 * TAUT_DEV_T and err_f <= 4 * TAUT_DEV_F
    assert n32[-1, 3] == 0.0 and np.all(np.abs(o32[0, 3:6].astype(np.float64) - want_t) <= 4 * TAUT_DEV_T)
    assert o32[0, 5] == n32[:-1, 3].max() and o32[0, 3] == n32[-2, 3] and o32[0, 4] == n32[0, 3]


def _settle(lines, attach, calls, dtype, watch=1, measure=None, **kw):
    """`calls` calls from reset: (nodes, line_out, [measure(nodes, line_out) after each of the last `watch` calls])."""
    nodes = M.reset(lines, attach)
    out, seen = None, []
    for k in range(calls):
        nodes, out, _ = M.mooring_step(lines, attach, nodes, None, 0, dtype=dtype, **kw)
        if measure is not None and k >= calls - watch:
            seen.append(measure(nodes, out))
    return nodes, out, np.array(seen)


# the largest |float32 - float64| of Fm.y + T0 e0.y over the last 100 calls of test_vertical_balance, measured
# once (N). One ulp of a node's position at |x| = 6 m is 4.8e-7 m, 1.2e-2 N on a segment of EA / l0 = 2.5e4 N/m:
# the float32 line keeps moving by that much around its rest.
BALANCE_DEV = 1.54e-3
BALANCE_CALLS = 400


def test_vertical_balance():
    """Both ends fixed 3 m apart at y = -5 in still water, a 4 m line of 6 nodes with linear drag: after settling,
    the pull on the fairlead plus the pull on the anchor carries the interior nodes' net weight,
    Fm.y + T0 e0.y = (n - 2) (mn g + rho_g vn), at every one of the last 100 calls."""
    n = 6
    lines = M.line((0.0, -5.0, 0.0), (3.0, -5.0, 0.0), 4.0, 2e4, 20.0, 2.0, 5e-4, 12.0, 0.0)[None]
    attach = np.array([[-1, n]], np.int32)
    c = M.constants(lines, attach)
    weight = (n - 2) * (float(c["mn"][0]) * float(F(-9.8)) + float(F(RHO_G)) * float(c["vn"][0]))

    def imbalance(nodes, out):
        e0 = (nodes[1, :3] - nodes[0, :3]).astype(np.float64)
        return float(out[0, 1]) + float(out[0, 4]) * e0[1] / np.linalg.norm(e0) - weight

    kw = dict(dt=1.0 / 30.0, rho_g=RHO_G, watch=100, measure=imbalance)
    n64, o64, i64 = _settle(lines, attach, BALANCE_CALLS, np.float64, **kw)
    n32, o32, i32 = _settle(lines, attach, BALANCE_CALLS, F, **kw)
    assert np.abs(i64).max() < 1e-9 and np.abs(n64[:, 4:7]).max() < 1e-10  # settled
    dev, err = float(np.abs(i32 - i64).max()), float(np.abs(i32).max())
    print(f"vertical balance over calls {BALANCE_CALLS - 100}..{BALANCE_CALLS}: net weight {weight:.6e} N, float32 - "
          f"float64 at most {dev:.3e} N, float32 imbalance at most {err:.3e} N (gate {4 * BALANCE_DEV:.3e}), sag "
          f"{-5.0 - n32[:, 1].min():.3f} m")
    assert err <= 4 * BALANCE_DEV
    assert np.all(n32[1:-1, 7] == 1.0) and o32[0, 7] == n - 2 and o32[0, 6] == 0.0 and n32[:, 1].min() < -5.5


# the largest |float32 - float64| of the resting penetration in test_node_rests_on_the_bed, measured once (m)
BED_DEV = 2.46e-7
BED_CALLS = 60


def test_node_rests_on_the_bed():
    """A slack 4 m line of 3 nodes with its ends 1 m apart at the bed's height: the middle node rests on the bed at
    pen = net weight / kb, the segments carry nothing."""
    bed_y, bed_k, bed_c = -1.0, 1e4, 2e2
    lines = M.line((0.0, bed_y, 0.0), (1.0, bed_y, 0.0), 4.0, 1e5, 0.0, 2.0, 5e-4)[None]
    attach = np.array([[-1, 3]], np.int32)
    c = M.constants(lines, attach)
    l0 = float(c["l0"][0])
    net = -(float(c["mn"][0]) * float(F(-9.8)) + float(F(RHO_G)) * float(c["vn"][0]))
    want = net / (float(F(bed_k)) * l0)
    kw = dict(rho_g=RHO_G, bed_y=bed_y, bed_k=bed_k, bed_c=bed_c)
    n64, o64, _ = _settle(lines, attach, BED_CALLS, np.float64, **kw)
    n32, o32, _ = _settle(lines, attach, BED_CALLS, F, **kw)
    pen64, pen32 = bed_y - n64[1, 1], float(F(bed_y)) - float(n32[1, 1])
    assert abs(pen64 - want) < 1e-12 and want > 0
    print(f"node on the bed after {BED_CALLS} calls: pen = {want:.6e} m, float32 - float64 {abs(pen32 - pen64):.3e} m, "
          f"float32 against the closed form {abs(pen32 - want):.3e} (gate {4 * BED_DEV:.3e})")
    assert abs(pen32 - want) <= 4 * BED_DEV
    assert n32[1, 7] == 3.0 and o32[0, 6] == 1.0 and o32[0, 7] == 1.0 and np.all(o32[0, :6] == 0.0)


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _layered(ocean, **overrides):
    """test_hulls._scene with the depth layers: (sampler, host maps, host rate maps, host layer maps)."""
    sampler, host, rates = _scene(ocean, 64, **overrides)
    gens = [g for g, _ in sampler.pairs]
    for g in gens:
        g.set_depth_layers(DEPTHS)
        g.calculate_kinematics()
    layers = [[(g.kinematics_map_host(0, l, 0), g.kinematics_map_host(0, l, 1)) for l in range(len(DEPTHS))] for g in gens]
    return sampler, host, rates, layers


@pytest.fixture(scope="module")
def calm64(ocean):
    return _layered(ocean)


@pytest.fixture(scope="module")
def steep64(ocean):
    return _layered(ocean, **STEEP)


BODIES = 6
LINE_BODIES = (0, -1, 1, 1, 1, 2, -1, 3, 0, -1, 2, 3)  # body 1 carries three lines, bodies 4 and 5 none
BED = dict(bed_y=-10.0, bed_k=2e4, bed_c=200.0)


def _lines(seed=12, counts=NODE_COUNTS, bodies=LINE_BODIES):
    """Lines of every count in NODE_COUNTS from anchors 12 m down (below the bed at -10 m) to fairleads on the
    random poses of test_hulls.py, or, without a body, to points 3 m above the water; some slack, some taut."""
    rng = np.random.default_rng(seed)
    poses = _random_poses(rng, BODIES)
    lines = np.zeros((len(counts), 16), F)
    for i, b in enumerate(bodies):
        if b >= 0:
            lf = rng.uniform(-1.0, 1.0, 3) * (2.0, 0.5, 4.0)
            top = poses[b, 9:12].astype(np.float64) + poses[b, :9].reshape(3, 3).astype(np.float64) @ lf
        else:
            lf = top = np.array([rng.uniform(-150, 150), 3.0, rng.uniform(-150, 150)])
        anchor = top + np.array([rng.uniform(-8, 8), 0.0, rng.uniform(-8, 8)])
        anchor[1] = -12.0
        span = float(np.linalg.norm(top - anchor))
        lines[i] = M.line(anchor, lf, span * (0.97 if i % 3 else 1.05), rng.uniform(2e4, 6e4), rng.uniform(0.0, 40.0),
                          rng.uniform(3.0, 8.0), rng.uniform(0.0, 2e-3), rng.uniform(0.0, 4.0), rng.uniform(0.0, 3.0))
    attach = np.stack([np.array(bodies, np.int32), np.array(counts, np.int32)], -1)
    return lines, attach, poses


def _mooring_set(sampler, lines, attach, bodies=BODIES):
    from oceansimulation_amd.surface import MooringSet

    return MooringSet(sampler.fft, lines, attach, bodies)


def _reset(moorings, poses):
    from oceansimulation_amd.hip import DeviceBuffer

    p = DeviceBuffer.from_array(np.ascontiguousarray(poses, F)) if poses is not None else None
    moorings.reset(p.ptr if p else 0)
    return moorings.nodes_host()


def _water_fn(oracle, scene, water, iterations, tolerance):
    _, host, _, layers = scene
    return M.water(oracle, host, layers, DEPTHS, iterations, tolerance) if water else M.still_water


def _check_calls(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert not np.isnan(w[0]).any() and not np.isnan(w[1]).any(), (what, "call", k, "the reference has NaN")
        for name, a, b in zip(("nodes", "line_out", "wrench_ext"), g, w):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, "call", k, name,
                                                                             float(np.nanmax(np.abs(a - b))))


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("water", [0, 1])
@pytest.mark.parametrize("scene_name", ["calm", "steep"])
def test_step_bit_exact(ocean, oracle, calm64, steep64, scene_name, water, substeps):
    """reset, then two successive calls on the device's own nodes, each compared with the restatement: nodes,
    line_out and wrench_ext (pre-filled with NaN), with every branch populated."""
    scene = calm64 if scene_name == "calm" else steep64
    iterations, tolerance = (4, 0.0) if scene_name == "calm" else (16, 1e-4)
    lines, attach, poses = _lines()
    moorings = _mooring_set(scene[0], lines, attach)
    start = _reset(moorings, poses)
    want_start = M.reset(lines, attach, poses)
    assert np.array_equal(_bits(start), _bits(want_start))
    kw = dict(dt=DT, substeps=substeps, rho_g=RHO_G, **BED)
    fn = _water_fn(oracle, scene, water, iterations, tolerance)
    want, nodes = [], want_start
    for _ in range(2):
        nodes, out, wrench = M.mooring_step(lines, attach, nodes, poses, BODIES, water_fn=fn, **kw)
        want.append((nodes, out, wrench))
    got = moorings.step_host(scene[0] if water else None, poses, calls=2, water=water, iterations=iterations,
                             tolerance=tolerance, **kw)
    _check_calls(got, want, f"{scene_name}, water {water}, {substeps} substeps")
    flags, T = want[-1][0][:, 7], want[-1][0][:, 3]
    interior = np.ones(len(flags), bool)
    offs = np.concatenate([[0], np.cumsum(attach[:, 1])])
    interior[offs[:-1]] = interior[offs[1:] - 1] = False
    assert set(np.unique(flags[interior])) == {0.0, 1.0, 3.0} and np.all(flags[~interior] == 0.0)  # dry, wet, wet on the bed
    assert (T > 0).any() and (want[-1][1][:, 5] == 0).any()  # taut and slack lines
    assert np.all(want[-1][2][[4, 5]] == 0.0) and want[-1][2][1, 3] == 3.0 and np.all(want[-1][2][:4, :3] != 0.0)
    assert not np.array_equal(want[0][0][:, :3], want_start[:, :3])
    moorings.close()


@pytest.mark.gpu
def test_reset_bit_exact_and_caller_nodes(ocean, calm64):
    """reset against the restatement; and nodes written by the caller are what the next step starts from."""
    lines, attach, poses = _lines(13)
    moorings = _mooring_set(calm64[0], lines, attach)
    assert moorings.lines == len(NODE_COUNTS) and moorings.total_nodes == sum(NODE_COUNTS)
    want = M.reset(lines, attach, poses)
    assert np.array_equal(_bits(_reset(moorings, poses)), _bits(want))
    rng = np.random.default_rng(3)
    moved = want.copy()
    moved[:, 0:3] += rng.uniform(-0.2, 0.2, (len(moved), 3)).astype(F)
    moved[:, 4:7] = rng.uniform(-1.0, 1.0, (len(moved), 3)).astype(F)
    moved[:, 3], moved[:, 7] = 7.0, 5.0  # not read
    moorings.set_nodes_host(moved)
    kw = dict(dt=DT, substeps=2, rho_g=RHO_G, **BED)
    got = moorings.step_host(None, poses, **kw)
    _check_calls(got, [M.mooring_step(lines, attach, moved, poses, BODIES, **kw)], "caller's nodes")
    moorings.close()


@pytest.mark.gpu
def test_replay_and_split_sets(ocean, calm64):
    """Two runs from the same state give the same bits; the same lines split into two sets give the same nodes
    and line_out (a line's result does not depend on its wave's other lines)."""
    sampler = calm64[0]
    lines, attach, poses = _lines(14)
    kw = dict(dt=DT, substeps=4, rho_g=RHO_G, water=1, **BED)

    def run(ln, at):
        m = _mooring_set(sampler, ln, at)
        _reset(m, poses)
        out = m.step_host(sampler, poses, calls=2, **kw)
        m.close()
        return out

    first, again = run(lines, attach), run(lines, attach)
    for a, b in zip(first, again):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    cut = 5  # between the packed pair (31, 32) and the 33-node line
    lo, hi = run(lines[:cut], attach[:cut]), run(lines[cut:], attach[cut:])
    rows = int(attach[:cut, 1].sum())
    for k in range(2):
        assert first[k][0][:rows].tobytes() == lo[k][0].tobytes() and first[k][0][rows:].tobytes() == hi[k][0].tobytes()
        assert first[k][1][:cut].tobytes() == lo[k][1].tobytes() and first[k][1][cut:].tobytes() == hi[k][1].tobytes()


# One wave (64 threads) per item: a workgroup is resident at most min(32, 2048 / 64) = 32 times per CU, so at
# budget 1 the grid has at most 32 workgroups and with 300 items some workgroup runs nine or more
# (tests/test_item_loops.py states the rule).
@pytest.mark.gpu
def test_budgeted_step_equals_full_device(ocean, calm64):
    sampler = calm64[0]
    rng = np.random.default_rng(300)
    counts = [40] * 300  # a wave each
    bodies = [int(b) for b in rng.integers(-1, BODIES, 300)]
    lines, attach, poses = _lines(301, counts, bodies)
    assert len(lines) >= 3 * 1 * min(32, 2048 // 64)
    kw = dict(dt=DT, substeps=3, rho_g=RHO_G, water=1, **BED)
    moorings = _mooring_set(sampler, lines, attach)
    try:
        _reset(moorings, poses)
        full = moorings.step_host(sampler, poses, calls=2, **kw)
        sampler.fft.set_cu_budget(1)
        one_start = _reset(moorings, poses)
        one = moorings.step_host(sampler, poses, calls=2, **kw)
    finally:
        sampler.fft.set_cu_budget(0)
    assert np.array_equal(_bits(one_start), _bits(M.reset(lines, attach, poses)))
    _check_calls(one, full, "budget 1 against the full device")
    assert (full[-1][1][:, 5] > 0).any()
    moorings.close()


def _moored_scene():
    """Four 16-point bodies of 500 kg at rest on the water; bodies 0 and 1 each on one taut line to an anchor
    20 m away against the push, body 2 on two, body 3 free (the control)."""
    rng = np.random.default_rng(40)
    points = _random_points(rng, 16)
    points[:, 3] = 1.0 / 16.0  # 1 m^3 of hull: half of it displaces the body's mass
    ranges = np.tile(np.array([[0, 16]], np.int32), (4, 1))
    poses = np.stack([H.pose(c=(40.0 * b - 60.0, 0.0, 15.0 * b)) for b in range(4)])
    props = np.stack([S.props(500.0, (300.0, 400.0, 500.0), 0.2, 0.5)] * 4)
    lines, attach = [], []
    for b, dz in ((0, 0.0), (1, 0.0), (2, 6.0), (2, -6.0)):
        lf = np.array([-1.0, 0.0, 0.0])
        top = poses[b, 9:12].astype(np.float64) + lf
        anchor = top + np.array([-16.0, -12.0, dz])
        # neutrally buoyant (rho_g vn = mn g), so the line stays straight and pulls from the first frame
        lines.append(M.line(anchor, lf, float(np.linalg.norm(top - anchor)), 2e5, 2e3, 5.0, 5.0 * 9.8 / RHO_G, 2.0, 1.0))
        attach.append((b, 8))
    return points, ranges, poses, props, np.stack(lines), np.array(attach, np.int32)


# The push: 2 m/s^2 of horizontal "gravity" on the hulls, 1000 N on 500 kg, for 5 frames of 0.2 s. Free, a body
# gains 0.5 * 2 * 1^2 = 1 m less what the hull drag takes (time constant > 1 s); moored, the line's
# EA / length = 1e4 N/m holds 1000 N at 0.1 m of stretch, at most twice that while it rings (w dt = 0.9 for
# 500 kg at dt = 0.2 s, inside the explicit coupling's stability limit of 2). 0.3 m separates the two.
DRIFT_BOUND = 0.3


@pytest.mark.gpu
def test_coupled_loop_with_hulls(ocean, oracle, calm64):
    """5 frames of moorings.step -> hulls.step(ext = wrench): poses and nodes equal the two restatements chained,
    and the moored bodies stay within DRIFT_BOUND of their start at every frame while the free control does not."""
    from oceansimulation_amd.hip import DeviceBuffer
    from oceansimulation_amd.surface import HullSet

    sampler, host, rates, layers = calm64
    points, ranges, poses, props, lines, attach = _moored_scene()
    mk = dict(dt=0.2, substeps=64, rho_g=RHO_G, water=1, iterations=4, tolerance=0.0)  # the bed far below
    hk = dict(dt=0.2, substeps=16, rho_g=RHO_G, water_velocity=1, gravity=(2.0, -9.8, 0.0))
    hulls = HullSet(sampler.fft, points, ranges)
    hulls.set_bodies(props)
    moorings = _mooring_set(sampler, lines, attach, 4)
    dev_poses = DeviceBuffer.from_array(poses)
    wrench, line_out = DeviceBuffer(4 * 8 * 4), DeviceBuffer(len(lines) * 8 * 4)
    moorings.reset(dev_poses.ptr)
    fn = M.water(oracle, host, layers, DEPTHS, 4, 0.0)
    loads_fn = S.water_loads(oracle, host, rates, points, ranges, RHO_G, 8, 0.0, True)
    want_poses, want_nodes = poses, M.reset(lines, attach, poses)
    moored, pull = 0.0, np.zeros(4, F)  # the largest drift, and the strongest pull against the push per body
    for frame in range(5):
        moorings.step(sampler, dev_poses.ptr, wrench.ptr, line_out.ptr, **mk)
        hulls.step(sampler, dev_poses.ptr, ext_ptr=wrench.ptr, **hk)
        want_nodes, want_lines, want_wrench = M.mooring_step(
            lines, attach, want_nodes, want_poses, 4, water_fn=fn,
            **{k: v for k, v in mk.items() if k not in ("water", "iterations", "tolerance")})
        want_poses, _, _ = S.hull_step(loads_fn, want_poses, props, hk["dt"], hk["substeps"], hk["gravity"], want_wrench)
        assert np.array_equal(_bits(moorings.nodes_host()), _bits(want_nodes)), frame
        assert np.array_equal(_bits(wrench.to_host((4, 8))), _bits(want_wrench)), frame
        assert np.array_equal(_bits(line_out.to_host((len(lines), 8))), _bits(want_lines)), frame
        assert np.array_equal(_bits(dev_poses.to_host((4, 20))), _bits(want_poses)), frame
        drift = np.linalg.norm((want_poses[:, [9, 11]] - poses[:, [9, 11]]).astype(np.float64), axis=1)
        moored, pull = max(moored, float(drift[:3].max())), np.minimum(pull, want_wrench[:, 0])
    print(f"horizontal drift over 5 frames of 0.2 s: moored at most {moored:.3f} m, free {drift[3]:.3f} m at the end "
          f"(bound {DRIFT_BOUND})")
    assert moored <= DRIFT_BOUND and drift[3] > DRIFT_BOUND
    assert pull[3] == 0.0 and np.all(pull[:3] < -500.0)  # every moored body was held back, by half the push at least
    assert want_wrench[3, 3] == 0.0 and want_wrench[2, 3] == 2.0 and want_wrench[0, 3] == 1.0
    moorings.close()
    hulls.close()


@pytest.mark.gpu
def test_kinematics_sampler_is_unchanged(ocean, oracle, steep64):
    """ocean_water_kinematics at the nodes of a reset set: the restatement's bits, as before its per-point body
    was shared with the mooring kernel."""
    sampler, host, _, layers = steep64
    lines, attach, poses = _lines(15)
    xyz = np.ascontiguousarray(M.reset(lines, attach, poses)[:, :3])
    got = sampler.kinematics_host(xyz, 16, 1e-4)
    assert np.array_equal(_bits(got), _bits(K.water_kinematics(oracle, host, layers, DEPTHS, xyz, 16, 1e-4)))
    assert set(np.unique(got[:, 11])) == {0.0, 1.0}


@pytest.mark.gpu
def test_invalid_step_calls_fail_loudly(ocean):
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.hip import DeviceBuffer
    from oceansimulation_amd.surface import SurfaceSampler

    fft = ocean.FFTCalculator(64)
    gens = [ocean.Generator(fft, 1) for _ in range(2)]
    for g in gens:
        g.CalculateOcean(1.0)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    lines = np.stack([M.line((0, -10, 0), (1, 0, 0), 12.0, 1e5, 10.0, 5.0, 1e-3, 1.0, 2.0)] * 2)
    attach = np.array([[0, 8], [-1, 5]], np.int32)
    poses = DeviceBuffer.from_array(H.pose()[None])
    wrench = DeviceBuffer(32)
    moorings = _mooring_set(sampler, lines, attach, 1)
    with pytest.raises(OceanError, match="ocean_moorings_step: the nodes were never reset nor written"):
        moorings.step(None, poses.ptr, wrench.ptr)
    with pytest.raises(OceanError, match="ocean_moorings_reset: null poses, and a line has a body"):
        moorings.reset(0)
    with pytest.raises(OceanError, match="never reset"):  # a refused reset places nothing
        moorings.step(None, poses.ptr, wrench.ptr)
    moorings.reset(poses.ptr)
    with pytest.raises(OceanError, match="ocean_moorings_step: null poses, and a line has a body"):
        moorings.step(None, 0, wrench.ptr)
    with pytest.raises(OceanError, match="ocean_moorings_step: null wrench_ext, and the set has bodies"):
        moorings.step(None, poses.ptr, 0)
    moorings.step(None, poses.ptr, wrench.ptr, substeps=256)  # still water: no generator, no line_out
    with pytest.raises(OceanError, match="ocean_moorings_step: .*pairs"):
        moorings.step(None, poses.ptr, wrench.ptr, water=1)
    with pytest.raises(OceanError, match="ocean_moorings_step: generator 0 has no depth layers"):
        moorings.step(sampler, poses.ptr, wrench.ptr, water=1)
    for g in gens:
        g.set_depth_layers(DEPTHS)
    gens[0].calculate_kinematics()
    with pytest.raises(OceanError, match="ocean_moorings_step: generator 1 has no depth layers"):
        moorings.step(sampler, poses.ptr, wrench.ptr, water=1)
    gens[1].set_depth_layers(DEPTHS[:3])
    gens[1].calculate_kinematics()
    with pytest.raises(OceanError, match="ocean_moorings_step: generator 1 has other depth layers than generator 0"):
        moorings.step(sampler, poses.ptr, wrench.ptr, water=1)
    gens[1].set_depth_layers(DEPTHS)
    gens[1].calculate_kinematics()
    moorings.step(sampler, poses.ptr, wrench.ptr, water=1)
    gens[0].CalculateOcean(2.0)
    with pytest.raises(OceanError, match="ocean_moorings_step: generator 0 has stale depth layers"):
        moorings.step(sampler, poses.ptr, wrench.ptr, water=1)
    foreign = ocean.Generator(ocean.FFTCalculator(64), 1)
    foreign.set_depth_layers(DEPTHS)
    foreign.CalculateOcean(1.0)
    foreign.calculate_kinematics()
    with pytest.raises(OceanError, match="ocean_moorings_step: the first generator is on another plan than the mooring set"):
        moorings.step(SurfaceSampler([(foreign, 0)]), poses.ptr, wrench.ptr, water=1)
    fft.synchronize()
    assert np.isfinite(moorings.nodes_host()).all() and np.isfinite(wrench.to_host((1, 8))).all()
    free = _mooring_set(sampler, lines[1:], np.array([[-1, 5]], np.int32), 0)  # no bodies: nothing but the set
    free.reset()
    free.step()
    assert free.step_host()[0][2].shape == (0, 8)
