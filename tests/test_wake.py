"""Wake windows (ocean_wake, include/oceanfft.h) against the contract restated in numpy (tests/wake_ref.py).

Every device comparison is bit for bit (view(np.uint32)): the contract fixes each rounding and the scatter is
integer, so there is no tolerance except on the taps, which are compared with a float64 quadrature at one float32
ulp.

Without a device the argument rules, the taps and the bound are reached through ocean_debug_wake_create_host, a
window without a plan: every rule of ocean_wake_step is checked before the window's storage is needed.

The item-loop cases. k_wake_substep has 256 threads and ceil(M / 32)^2 items, k_wake_splat 256 threads and
ceil(records / 256) items; tests/test_item_loops.py's condition for "some workgroup runs three or more items" is
items >= 3 * budget * min(32, 2048 / 256). M = 80 (9 tiles) and 3000 records (12 items) are the sizes the other
tests use and loop under a budget only where fewer than 9 (12) workgroups are resident; M = 224 (49 tiles) with
12500 records (49 items) satisfies the condition at budgets 1 and 2 whatever the occupancy, so both are run.
h_prev is an input of a substep (the new h is written over it), so it cannot be filled with 0xFF bytes: a NaN there
is the result everywhere. What the sentinel is for, a skipped item that passes on recycled memory, is covered
otherwise: the budgeted window lives on a plan of its own beside the full-device one, and a skipped tile keeps the
h of two substeps earlier, which for the random field differs from the new h in every texel.
"""
import ctypes
import os

import numpy as np
import pytest

import wake_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
F = np.float32
DX = 0.25
OX, OZ = -3.5, 2.25
NEW_CALLS = ("ocean_wake_create", "ocean_wake_destroy", "ocean_wake_size", "ocean_wake_kernel",
             "ocean_wake_max_substep", "ocean_wake_origin", "ocean_wake_height", "ocean_wake_reset", "ocean_wake_shift",
             "ocean_default_wake_settings", "ocean_wake_step", "ocean_wake_sample", "ocean_debug_wake_create_host")
STEP = dict(damp=0.05, edge_damp=4.0, border=8, gravity=9.8, rho_g=9810.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


# ---- without a GPU ------------------------------------------------------------------------------------
def test_exports_defaults_and_header():
    import oceansimulation_amd as ocean
    from oceansimulation_amd import capi, wake

    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "oceanfft.h")).read()
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi.SIGNATURES and name + "(" in header, name
    for name in ("Wake", "OceanWakeSettings", "default_wake_settings", "apply_wake_settings"):
        assert hasattr(ocean, name) and name in ocean.__all__, name
    for name in ("create", "reset", "shift", "step", "step_ptr", "sample_ptr", "sample_host", "height", "kernel", "max_substep"):
        assert name == "create" or hasattr(wake.Wake, name), name
    assert ctypes.sizeof(capi.OceanWakeSettings) == 32
    s = capi.OceanWakeSettings(*([-1] * 7))
    L.ocean_default_wake_settings(ctypes.byref(s))
    got = (s.dt, s.substeps, s.gravity, s.rho_g, s.damp, s.edge_damp, s.border)
    assert got == (F(1.0 / 60.0), 4, F(9.8), F(9810.0), F(0.05), F(8.0), 16)
    names = ("dt", "substeps", "gravity", "rho_g", "damp", "edge_damp", "border")
    assert [float(g) for g in got] == [float(F(W.DEFAULTS[k])) for k in names]
    L.ocean_default_wake_settings(None)  # a null output is ignored
    s = ocean.default_wake_settings(substeps=2, damp=0.5)
    assert (s.substeps, s.damp, s.border) == (2, 0.5, 16)
    with pytest.raises(AttributeError):
        ocean.apply_wake_settings(s, gain=1.0)
    body = header[header.index("typedef struct ocean_wake_settings"):header.index("} ocean_wake_settings;")]
    fields = [f[0] for f in capi.OceanWakeSettings._fields_]
    assert sorted(fields, key=lambda f: body.index(f" {f};")) == fields
    assert header.index("ocean_moorings_step(") < header.index("---- Wake windows") < header.index("---- Persistent foam")
    assert header.index("---- Wake windows") < header.index("typedef struct ocean_wake_settings")
    for text in ("No reference counterpart", "h_tt = -(g / dx) G * (h + P)", "A[t] += (int64)(p' * 1048576.0f)",
                 "h_new[t] = (((2.0f * h[t]) - (1.0f - b) * h_prev[t]) - c * acc) / (1.0f + b)",
                 "waves longer\n * than about 30 texels travel too fast", "at most substeps + 2"):
        assert text in header, text
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert "launch_wake" in makefile[makefile.index("KERNEL_TUS :="):makefile.index("KERNEL_OBJS :=")]
    for name in ("device/k_wake.h", "launch_wake.hip"):
        assert os.path.exists(os.path.join(ROOT, "oceansimulation_amd", "csrc", name)), name
    kernels = open(os.path.join(ROOT, "oceansimulation_amd", "csrc", "device", "k_wake.h")).read()
    for name in ("k_wake_splat", "k_wake_substep", "k_wake_shift", "k_wake_sample"):
        assert name in kernels, name
    assert "persistent_grid(k_wake_substep" in open(os.path.join(ROOT, "oceansimulation_amd", "csrc", "launch_wake.hip")).read()


@pytest.mark.parametrize("sigma", [0.3, 0.5, 0.55])
def test_taps_match_the_quadrature(sigma):
    """The library's taps, built without a device, against the float64 Gauss-Legendre quadrature of the defining
    integral: within one float32 ulp of the rounded float64 value; symmetric; positive symbol; the bound."""
    import oceansimulation_amd as ocean

    w = ocean.Wake(None, 64, DX, OX, OZ, sigma)
    t = w.kernel()
    assert t.dtype == F and t.shape == (7, 7) and np.array_equal(t, t.T)
    want = W.taps_quadrature(float(F(sigma))).astype(F)  # the smoothing is a float argument
    ulps = np.abs(t.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert np.all(np.sign(t) == np.sign(want)) and ulps.max() <= 1, ulps
    assert W.symbol_min(t) > 0.0
    for gravity in (9.8, 1.62):
        got, ref = w.max_substep(gravity), W.max_substep(t, DX, gravity)
        assert abs(got - ref) <= 1e-12 * ref, (got, ref)
    if sigma == 0.5:
        assert abs(w.max_substep(9.8) - 0.29) < 0.005  # the header's figure
        d = ocean.Wake(None, 64, DX, OX, OZ, 0.0)  # 0: the default
        assert np.array_equal(d.kernel(), t)
        d.close()
    assert w.origin() == (OX, OZ) and w.size == 64
    w.close()


def test_rejected_arguments_name_the_call():
    """Everything that can be refused without a device: OCEAN_ERR_INVALID with the entry point's name and the field
    in ocean_last_error. The plan and the records are pointers that are never dereferenced; a step with good
    arguments stops at the host-only window's missing storage."""
    from oceansimulation_amd import capi

    L = capi.lib()
    inv = capi.OCEAN_ERR_INVALID
    one = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
    nan, inf = float("nan"), float("inf")

    def create(out=True, fft=one, size=64, dx=DX, ox=0.0, oz=0.0, sigma=0.5):
        h = ctypes.c_void_p()
        return L.ocean_wake_create(ctypes.byref(h) if out else None, fft, size, dx, ox, oz, sigma)

    for kwargs, word in [(dict(out=False), b"null"), (dict(fft=None), b"null"), (dict(size=16), b"size"),
                         (dict(size=72), b"size"), (dict(size=4112), b"size"), (dict(size=-64), b"size"),
                         (dict(dx=0.0), b"dx"), (dict(dx=-1.0), b"dx"), (dict(dx=nan), b"dx"), (dict(dx=inf), b"dx"),
                         (dict(ox=nan), b"origin"), (dict(oz=-inf), b"origin"), (dict(sigma=0.6), b"smoothing"),
                         (dict(sigma=0.29), b"smoothing"), (dict(sigma=nan), b"smoothing"), (dict(sigma=-0.5), b"smoothing")]:
        assert create(**kwargs) == inv, kwargs
        assert b"ocean_wake_create:" in L.ocean_last_error() and word in L.ocean_last_error(), (kwargs, L.ocean_last_error())

    h = ctypes.c_void_p()
    assert L.ocean_debug_wake_create_host(ctypes.byref(h), 64, DX, 0.0, 0.0, 0.5) == capi.OCEAN_OK
    bound = L.ocean_wake_max_substep(h, 9.8)
    at_bound = float(np.nextafter(F(bound), F(1.0)) if float(F(bound)) < bound else F(bound))  # the first float >= it
    assert at_bound >= bound > float(np.nextafter(F(at_bound), F(0.0)))

    def step(wake=h, settings=True, records=one, count_device=None, max_records=4, **fields):
        s = capi.OceanWakeSettings()
        L.ocean_default_wake_settings(ctypes.byref(s))
        for k, v in fields.items():
            setattr(s, k, v)
        return L.ocean_wake_step(wake, ctypes.byref(s) if settings else None, records, count_device,
                                 ctypes.c_int64(max_records))

    cases = [(dict(wake=None), b"null wake"), (dict(settings=False), b"null settings"),
             (dict(dt=0.0), b"dt"), (dict(dt=-1.0), b"dt"), (dict(dt=nan), b"dt"), (dict(dt=inf), b"dt"),
             (dict(substeps=0), b"substeps"), (dict(substeps=65), b"substeps"),
             (dict(gravity=0.0), b"gravity"), (dict(gravity=-9.8), b"gravity"), (dict(gravity=nan), b"gravity"),
             (dict(gravity=inf), b"gravity"), (dict(rho_g=0.0), b"rho_g"), (dict(rho_g=nan), b"rho_g"), (dict(rho_g=inf), b"rho_g"),
             (dict(damp=-0.1), b"damp"), (dict(damp=nan), b"damp"), (dict(damp=inf), b"damp"),
             (dict(edge_damp=-0.1), b"edge_damp"), (dict(edge_damp=nan), b"edge_damp"), (dict(edge_damp=inf), b"edge_damp"),
             (dict(border=-1), b"border"), (dict(border=33), b"border"),
             (dict(max_records=-1), b"max_records"), (dict(max_records=(1 << 28) + 1), b"max_records"),
             (dict(records=None), b"null records"),
             (dict(dt=at_bound, substeps=1), b"ocean_wake_max_substep"), (dict(dt=8 * at_bound, substeps=8), b"ocean_wake_max_substep"),
             (dict(dt=1.0, substeps=1), b"ocean_wake_max_substep"),
             # accepted values, refused only for the storage this window does not have
             (dict(dt=float(np.nextafter(F(at_bound), F(0.0))), substeps=1), b"no device storage"),
             (dict(border=0), b"no device storage"), (dict(border=32), b"no device storage"),
             (dict(records=None, max_records=0), b"no device storage"), (dict(max_records=1 << 28), b"no device storage"),
             (dict(count_device=one), b"no device storage"), (dict(damp=0.0, edge_damp=0.0), b"no device storage"),
             (dict(substeps=64, dt=1.0), b"no device storage"), (dict(), b"no device storage")]
    for kwargs, word in cases:
        assert step(**kwargs) == inv, (kwargs, word)
        assert b"ocean_wake_step:" in L.ocean_last_error() and word in L.ocean_last_error(), (kwargs, L.ocean_last_error())

    for call, args, word in [(L.ocean_wake_sample, (None, one, 1, one), b"null wake"),
                             (L.ocean_wake_sample, (h, one, -1, one), b"n outside"),
                             (L.ocean_wake_sample, (h, one, 1 << 31, one), b"n outside"),
                             (L.ocean_wake_sample, (h, None, 1, one), b"null xz"),
                             (L.ocean_wake_sample, (h, one, 1, None), b"null xz"),
                             (L.ocean_wake_sample, (h, one, 1, one), b"no device storage"),
                             (L.ocean_wake_shift, (None, 0, 0), b"null wake"),
                             (L.ocean_wake_shift, (h, (1 << 20) + 1, 0), b"di or dj"),
                             (L.ocean_wake_shift, (h, 0, -(1 << 20) - 1), b"di or dj"),
                             (L.ocean_wake_shift, (h, 1, 1), b"no device storage"),
                             (L.ocean_wake_reset, (None,), b"null wake"), (L.ocean_wake_reset, (h,), b"no device storage"),
                             (L.ocean_wake_kernel, (None, (ctypes.c_float * 49)()), b"null"),
                             (L.ocean_wake_kernel, (h, None), b"null"), (L.ocean_wake_origin, (h, None), b"null")]:
        assert call(*args) == inv, (call.__name__, args)
        assert call.__name__.encode() + b":" in L.ocean_last_error() and word in L.ocean_last_error(), L.ocean_last_error()
    assert not L.ocean_wake_height(None) and not L.ocean_wake_height(h) and L.ocean_wake_size(None) == 0
    assert L.ocean_wake_max_substep(None, 9.8) == 0.0 and L.ocean_wake_max_substep(h, 0.0) == 0.0
    assert L.ocean_wake_destroy(h) == capi.OCEAN_OK and L.ocean_wake_destroy(None) == capi.OCEAN_OK


@pytest.fixture(scope="module")
def taps():
    import oceansimulation_amd as ocean

    w = ocean.Wake(None, 64, DX, 0.0, 0.0, 0.5)
    t = w.kernel()
    w.close()
    return t


def test_scheme_impulse_stays_bounded(taps):
    """(a) A unit impulse at the centre, 400 substeps at 0.9 of the bound without interior damping: the waves leave
    through the absorbing frame and nothing grows. Measured here: 1.53 over substeps 0..49, 0.089 over 350..399."""
    win = W.Window(64, DX, 0.0, 0.0, taps)
    win.h[32, 32] = 1.0
    hs = 0.9 * W.max_substep(taps, DX, 9.8)
    peaks = []
    for _ in range(400):
        win.step(dt=hs, substeps=1, damp=0.0, edge_damp=4.0, border=8)
        peaks.append(float(np.abs(win.h).max()))
    print("peaks", max(peaks[:50]), max(peaks[350:]))
    assert np.isfinite(peaks).all() and max(peaks[350:]) <= max(peaks[:50])


def test_scheme_constant_patch_settles_to_minus_p(taps):
    """(b) h = -P is the fixed point: a constant 4 x 4 patch of P = 0.1, damp 0.5, hs = 0.05, 2000 substeps.
    Measured here: 7.7e-7 (the float32 resolution of the patch sum sets the floor)."""
    win = W.Window(64, DX, 0.0, 0.0, taps)
    p = np.zeros((64, 64), F)
    p[30:34, 30:34] = 0.1
    for _ in range(2000):
        new = W.substep(win.h, win.h_prev, p, win.taps, win.dx, 0.05, 9.8, 0.5, 4.0, 8)
        win.h_prev, win.h = win.h, new
    worst = float(np.abs(win.h + p).max())
    print("max |h + P|", worst)
    assert worst < 1e-5


def _records(m, count, seed, pile=300):
    """Rows in the layout of point_out over [ox - 2 dx, ox + (M + 1) dx]^2 (every edge-drop case), `pile` of them on
    one texel, F of both signs with one NaN, +inf, -inf and values that hit the clamp."""
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((count, 8)).astype(F)
    rec[:, 0] = rng.uniform(OX - 2 * DX, OX + (m + 1) * DX, count)
    rec[:, 2] = rng.uniform(OZ - 2 * DX, OZ + (m + 1) * DX, count)
    rec[:, 5] = rng.standard_normal(count) * 40.0
    where = rng.choice(count - 100, pile, replace=False)
    rec[where, 0] = OX + (20 + rng.uniform(0.0, 1.0, pile)) * DX
    rec[where, 2] = OZ + (41 + rng.uniform(0.0, 1.0, pile)) * DX
    inside = [k for k in range(count - 100) if k not in set(where)][:8]
    for k, f in zip(inside, (np.nan, np.inf, -np.inf, 3e9, -3e9, 1e12, -1e12, 6.5e8)):
        rec[k, 0] = OX + (10.3 + 5 * inside.index(k)) * DX
        rec[k, 2] = OZ + 17.6 * DX
        rec[k, 5] = f
    rec[5, 0], rec[6, 2] = np.nan, np.nan  # culled
    return rec


def test_scheme_splat_is_order_independent(taps):
    """(c) A permuted record list gives identical accumulators; the specials land as the contract says."""
    win = W.Window(64, DX, OX, OZ, taps)
    rec = _records(64, 3000, seed=1)
    a = W.splat(win, rec, 2900)
    perm = np.random.default_rng(2).permutation(2900)
    assert np.array_equal(a, W.splat(win, rec[perm], 2900))
    assert not np.array_equal(a, W.splat(win, rec, 3000))
    assert (a[41:43, 20:22] != 0).all() and np.abs(a).max() >= 1 << 40  # the pile; a clamped tap
    assert (a != 0).sum() > 2000 and a[0].any() and a[-1].any() and a[:, 0].any() and a[:, -1].any()


def test_scheme_shift_restores_the_interior():
    """(d) Shift by (3, -5) and then (-3, 5): the interior is restored and the exposed strips are zero."""
    rng = np.random.default_rng(3)
    a = rng.standard_normal((64, 64)).astype(F)
    b = W.shifted(W.shifted(a, 3, -5), -3, 5)
    assert np.array_equal(b[:59, 3:], a[:59, 3:]) and not b[59:].any() and not b[:, :3].any()
    once = W.shifted(a, 3, -5)
    assert once[10, 7] == a[5, 10] and not once[:, 61:].any() and not once[:5].any()
    assert not W.shifted(a, -64, 0).any() and np.array_equal(W.shifted(a, 0, 0), a)


# ---- on the GPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


@pytest.fixture(scope="module")
def fft(ocean):
    return ocean.FFTCalculator(64)


def _field(m, seed):
    return (np.random.default_rng(seed).standard_normal((m, m)) * 0.1).astype(F)


def _loaded(ocean, fft, m, seed=7):
    """A device window and its restatement, h loaded with a random field and one first step taken, so that h_prev is
    a random field too."""
    from oceansimulation_amd import hip

    wake = ocean.Wake(fft, m, DX, OX, OZ, 0.5)
    ref = W.Window(m, DX, OX, OZ, wake.kernel())
    _load(wake, ref, _field(m, seed))
    return wake, ref


def _load(wake, ref, field):
    from oceansimulation_amd import hip

    wake.reset()
    wake.fft.synchronize()
    hip.from_host(wake.height_ptr(), field)
    ref.reset()
    ref.h = field.copy()
    _same(wake.step_host(dt=0.05, substeps=1, **STEP), _ref_step(ref, dt=0.05, substeps=1), "first step")


def _ref_step(ref, records=None, count=None, **kw):
    ref.step(records, count, **dict(STEP, **kw))
    return ref.h


@gpu
@pytest.mark.parametrize("m", [64, 80])
def test_substep_alone_bit_exact(ocean, fft, m):
    """No records: 1 and then 5 substeps from random h and h_prev, the whole map, border and corners included."""
    wake, ref = _loaded(ocean, fft, m)
    for substeps in (1, 5):
        got = wake.step_host(dt=0.05 * substeps, substeps=substeps, **STEP)
        _same(got, _ref_step(ref, dt=0.05 * substeps, substeps=substeps), f"{substeps} substeps")
    assert np.isfinite(ref.h).all() and np.abs(ref.h).max() > 1e-3
    wake.close()


@gpu
def test_splat_and_substep_bit_exact(ocean, fft):
    """3000 fabricated records of which the device count admits 2900: maps bit exact, the accumulators zero again
    (a following call with a device count of 0 reads them), the permuted list and a replay give the same bytes."""
    m = 64
    rec = _records(m, 3000, seed=1)
    wake, ref = _loaded(ocean, fft, m)
    start = _field(m, 7)
    kw = dict(dt=0.1, substeps=4)
    first = wake.step_host(rec, 2900, **dict(STEP, **kw)).copy()
    acc = ref.step(rec, 2900, **dict(STEP, **kw))
    assert np.abs(acc).max() >= 1 << 40 and (acc != 0).sum() > 2000
    _same(first, ref.h, "splat + 4 substeps")
    after = wake.step_host(rec, 0, **dict(STEP, **kw))  # P = 0 only if every accumulator is zero again
    _same(after, _ref_step(ref, None, **kw), "a call that reads the accumulators after the splat")
    perm = np.random.default_rng(2).permutation(2900)
    shuffled = np.concatenate([rec[perm], rec[2900:]])
    for what, records in (("permuted", shuffled), ("replay", rec)):
        _load(wake, ref, start)
        _same(wake.step_host(records, 2900, **dict(STEP, **kw)), first, what)
    _load(wake, ref, start)
    _same(wake.step_host(rec[:2900], None, **dict(STEP, **kw)), first, "a null count_device")
    wake.close()


@gpu
def test_hull_coupling_bit_exact(ocean):
    """test_hull_step.py's scene (three cascades at N = 64), two bodies of 16 points and one of 80: five frames of
    ocean_hulls_step with point_out, each followed by ocean_wake_step (4 substeps) on that point_out. The restatement
    is fed the device's own point_out bytes of each frame; h after every frame is bit exact, and after frame 5 it is
    non-zero under every body."""
    import hull_loads_ref as H
    from oceansimulation_amd.hip import DeviceBuffer
    from oceansimulation_amd.surface import HullSet
    from test_hulls import _random_points, _scene
    from test_hull_step import _random_props

    sampler, _, _ = _scene(ocean, 64)
    rng = np.random.default_rng(11)
    points = _random_points(rng, 96)
    ranges = np.array([(0, 16), (16, 16), (16, 80)], np.int32)
    centres = [(4.0, -0.1, 5.0), (12.0, 0.0, 4.0), (8.0, -0.2, 10.5)]
    poses = np.stack([H.pose(None, c, (1.0, 0.0, 0.5), (0.0, 0.1, 0.0)) for c in centres])
    hulls = HullSet(sampler.fft, points, ranges)
    hulls.set_bodies(_random_props(rng, points, ranges))
    assert hulls.instance_points == 112
    wake = ocean.Wake(sampler.fft, 64, DX, 0.0, 0.0, 0.5)
    ref = W.Window(64, DX, 0.0, 0.0, wake.kernel())
    pose_buf = DeviceBuffer.from_array(poses)
    pts = DeviceBuffer(112 * 32)
    kw = dict(dt=1.0 / 60.0, substeps=4)
    for frame in range(5):
        hulls.step(sampler, pose_buf.ptr, point_out_ptr=pts.ptr, dt=1.0 / 60.0, substeps=1)
        wake.step_ptr(pts.ptr, 112, 0, **dict(STEP, **kw))
        got = wake.height_host()
        rows = pts.to_host((112, 8))
        _same(got, _ref_step(ref, rows, **kw), f"frame {frame}")
    first = 0
    for b, (_, count) in enumerate(ranges):
        r = rows[first:first + count]
        first += count
        i = np.clip(np.floor(r[:, 0] / DX).astype(int), 0, 63)
        j = np.clip(np.floor(r[:, 2] / DX).astype(int), 0, 63)
        assert (r[:, 5] != 0).any() and (got[j, i] != 0).any(), b
    hulls.close()
    wake.close()


def _sample_points(m, seed):
    rng = np.random.default_rng(seed)
    xz = np.empty((4096, 2), F)
    xz[:, 0] = rng.uniform(OX - 3 * DX, OX + (m + 2) * DX, 4096)
    xz[:, 1] = rng.uniform(OZ - 3 * DX, OZ + (m + 2) * DX, 4096)
    k = np.arange(m)
    xz[:m, 0], xz[:m, 1] = OX + k * DX, OZ + ((k * 7) % m) * DX  # exact texel centres
    xz[m:2 * m, 0], xz[m:2 * m, 1] = OX + (m - 1) * DX, OZ + np.minimum(k + 0.25, m - 1) * DX  # the last column
    xz[2 * m:3 * m, 0], xz[2 * m:3 * m, 1] = OX + np.minimum(k + 0.5, m - 1) * DX, OZ + (m - 1) * DX  # the last row
    xz[3 * m:4 * m, 0], xz[3 * m:4 * m, 1] = OX + m * DX, OZ + k * DX  # one texel outside
    xz[4 * m:5 * m, 0], xz[4 * m:5 * m, 1] = OX + k * DX, OZ - DX
    xz[5 * m, 0], xz[5 * m + 1, 1], xz[5 * m + 2] = np.nan, np.nan, (np.inf, OZ)
    return xz


@gpu
@pytest.mark.parametrize("m", [64, 80])
def test_shift_and_sample_bit_exact(ocean, fft, m):
    """Samples before any step (dh/dt = 0) and after one; shifts (3, -5), (0, 0) and (-M, 0) of both maps, seen through
    h, the origin, the samples (h - h_prev) and one more substep."""
    from oceansimulation_amd import hip

    wake = ocean.Wake(fft, m, DX, OX, OZ, 0.5)
    ref = W.Window(m, DX, OX, OZ, wake.kernel())
    xz = _sample_points(m, seed=5)
    field = _field(m, 9)
    fft.synchronize()
    hip.from_host(wake.height_ptr(), field)
    ref.h = field.copy()
    before = wake.sample_host(xz)
    _same(before, ref.sample(xz), "samples before any step")
    assert not before[:, 3].any() and before[:, 0].any()
    _same(wake.step_host(dt=0.05, substeps=1, **STEP), _ref_step(ref, dt=0.05, substeps=1))
    got = wake.sample_host(xz)
    _same(got, ref.sample(xz), "samples after a step")
    assert got[:m, 3].any() and not got[3 * m:5 * m + 3].any() and got[m:3 * m, 0].all()
    for di, dj in ((3, -5), (0, 0)):
        wake.shift(di, dj)
        ref.shift(di, dj)
        _same(wake.height_host(), ref.h, f"shift {(di, dj)}")
        assert wake.origin() == (float(ref.ox()), float(ref.oz()))
        _same(wake.sample_host(xz), ref.sample(xz), f"samples after shift {(di, dj)}")
    assert wake.origin() == (float(F(OX + F(3 * DX))), float(F(OZ - F(5 * DX))))
    rec = _records(m, 500, seed=4, pile=50)
    _same(wake.step_host(rec, **dict(STEP, dt=0.05, substeps=1)), _ref_step(ref, rec, dt=0.05, substeps=1),
          "a forced substep after the shift: h_prev moved with h, the accumulators are zero")
    wake.shift(-m, 0)
    ref.shift(-m, 0)
    assert not wake.height_host().any() and not ref.h.any()
    _same(wake.sample_host(xz), ref.sample(xz), "samples of the cleared window")
    assert not ref.h_prev.any()
    wake.reset()
    ref.reset()
    assert not wake.sample_host(xz).any()
    wake.close()


def _max_resident(wg):
    return min(32, 2048 // wg)


def _bound_holds(wg, items, budget):
    """tests/test_item_loops.py's condition: some workgroup of a budgeted grid runs three or more items."""
    return items >= 3 * budget * _max_resident(wg)


@gpu
@pytest.mark.parametrize("m, count", [(80, 3000), (224, 12500)])
def test_budgeted_steps_equal_full_device(ocean, fft, m, count):
    """The 5-substep and the splat cases at CU budgets 1 and 2, on windows and plans of their own, against the full
    device's bytes and the restatement (module docstring)."""
    tiles = (-(-m // 32)) ** 2
    items = -(-count // 256)
    if m == 224:
        for b in (1, 2):
            assert _bound_holds(256, tiles, b) and _bound_holds(256, items, b)
    rec = _records(m, count, seed=6)
    results = []
    for budget in (0, 1, 2):
        plan = fft if budget == 0 else ocean.FFTCalculator(64)
        plan.set_cu_budget(budget)
        try:
            wake, ref = _loaded(ocean, plan, m)
            free = wake.step_host(dt=0.25, substeps=5, **STEP).copy()
            forced = wake.step_host(rec, count - 100, **dict(STEP, dt=0.1, substeps=4)).copy()
            again = wake.step_host(rec, 0, **dict(STEP, dt=0.05, substeps=1)).copy()
            results.append((free, forced, again))
            wake.close()
        finally:
            plan.set_cu_budget(0)
    want = (_ref_step(ref, dt=0.25, substeps=5).copy(), _ref_step(ref, rec, count - 100, dt=0.1, substeps=4).copy(),
            _ref_step(ref, None, dt=0.05, substeps=1).copy())
    for budget, got in zip((0, 1, 2), results):
        for name, a, b in zip(("5 substeps", "splat", "after the splat"), got, want):
            _same(a, b, (budget, name))


@gpu
def test_steps_allocate_nothing(ocean, fft):
    """hipMemGetInfo's free memory is equal before and after 10 steps with records, shifts and samples."""
    from oceansimulation_amd import hip
    from oceansimulation_amd.hip import DeviceBuffer

    h = hip.hip()
    h.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    h.hipMemGetInfo.restype = ctypes.c_int

    def free_bytes():
        fft.synchronize()
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert h.hipMemGetInfo(ctypes.byref(a), ctypes.byref(b)) == 0
        return a.value

    wake = ocean.Wake(fft, 80, DX, OX, OZ, 0.5)
    rec = DeviceBuffer.from_array(_records(80, 3000, seed=8))
    cnt = DeviceBuffer.from_array(np.array([2900], np.int64))
    xz = DeviceBuffer.from_array(_sample_points(80, seed=5))
    out = DeviceBuffer(4096 * 16)
    kw = dict(STEP, dt=0.1, substeps=4)

    def frame():
        wake.step_ptr(rec.ptr, 3000, cnt.ptr, **kw)
        wake.step_ptr(**kw)
        wake.shift(1, -1)
        wake.sample_ptr(xz.ptr, 4096, out.ptr)

    frame()  # the kernels' code objects are loaded
    before = free_bytes()
    for _ in range(10):
        frame()
    assert free_bytes() == before
    assert np.isfinite(wake.height_host()).all()
    wake.close()
