"""Parity away from the default settings: the spectral peak inside the grid, finite depth, another gravity and
wind direction, the spreading function's two ends, settings edited between frames, and batches whose cascades
differ in more than plane and seed (tests/settings_cases.py for the cases and what each is there to reach).

The CPU tests make the coverage a condition and pin the two references (oracle, numpy_ref) on each other at
every (case, N) the GPU tests run. The GPU tests then repeat the default-settings checks of test_gpu_parity.py
and test_rates.py at those settings, with their gates (tests/parity.py) and their checkers unchanged.

Time and finite depth: where k h < 2 pi the frequency w depends on a float32 tanh, which the oracle (libm),
numpy_ref and the device (1 - 2 / (1 + e^{2kh}), an odd series below 1/8) round differently by ulps; the phase
w t multiplies that by t. The two references' prepared spectra differ by 1.4-4.7e-7 at t = 1, 1.3-4.5e-5 at
t = 100 and 1.1-3.7e-4 at t = 1000 (CPU, lane_err). So the finite-depth frames run at t ~ 1, where that noise is
far under the gates; one test looks at t = 100 with a gate that measures the noise itself; the deep-water
cases (tanh = 1, w bit-identical to the oracle's) run to t = 3600 at the plain gates.
"""
import numpy as np
import pytest

import numpy_ref as R
import settings_cases as SC
from parity import FRAME_TOL_GPU, H0_TOL, channel_err, lane_err, scalar_err
from test_gpu_parity import _f64_frame, _frame_check, _slab_run
from test_rates import _rate_errs

CASE_NAMES = list(SC.CASES)
MIXED = ("default", "peak", "shallow", "light_gravity")  # the mixed batch's cascades
# every (case, N) a GPU test below runs
PAIRS = ([(name, n) for name in CASE_NAMES for n in (64, 1024)] + [("default", 64), ("default", 1024),
                                                                    ("peak_shallow", 256)])
SMALL_T = (1.0, 1.0 / 60.0)

_cache = {}


def _shared(key, make):
    """A reference computed once and shared by the tests that need it (nobody writes to it)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _spectra(oracle, name, n):
    """(oracle h0, numpy_ref h0) at the case's settings."""
    def make():
        s = oracle.default_settings(**SC.settings(name, n))
        return oracle.generate_spectrum(s, n), R.generate_spectrum(s, n)

    return _shared(("h0", name, n), make)


def _k_index(n):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.hypot(x - n / 2, y - n / 2)[..., None]


def _h0_errs(got, ref):
    """(plain, weighted by |k| in texels) lane errors, as test_generate_spectrum."""
    k = _k_index(ref.shape[0])
    return max(lane_err(got, ref)), max(lane_err(got * k, ref * k))


# ---- without a GPU ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", PAIRS)
def test_cases_reach_their_branches(oracle, name, n):
    """Each share of the grid a case is there for holds >= 1 % of the texels at every size it runs at, the
    deep-water cases keep tanh = 1 on every texel at N = 64 (test_deep_water_stays_exact_long_time depends on
    it), and the references are finite there (a 0/0 at the peak or an overflowing e^{2kh} would show here)."""
    cov = SC.coverage(SC.settings(name, n), n)
    print(name, n, {k: round(v, 4) for k, v in cov.items()})
    for key in SC.REACHES.get(name, ()):
        assert cov[key] >= SC.MIN_SHARE, (name, n, key, cov[key])
    if n == 64 and (name in SC.DEEP or name == "default"):
        assert cov["tanh_series"] == 0.0 and cov["tanh_exp"] == 0.0, cov
    h0, h0_np = _spectra(oracle, name, n)
    assert np.isfinite(h0).all() and np.isfinite(h0_np).all()
    s = oracle.default_settings(time=1.0, **SC.settings(name, n))
    for img in oracle.prepare_fft(s, n, h0) + R.prepare_fft(s, n, h0):
        assert np.isfinite(img).all()


def test_default_suite_settings_reach_none_of_them():
    """What the other modules run (defaults on 40 m, N = 64): nothing of the above."""
    assert set(SC.coverage(dict(planeSize=40.0), 64).values()) == {0.0}


@pytest.mark.parametrize("name,n", PAIRS)
def test_references_agree_on_h0(oracle, name, n):
    """Oracle against numpy_ref, written separately from the GLSL: measured on the CPU <= 1.7e-6 plain and
    <= 1.7e-6 weighted over these pairs."""
    h0, h0_np = _spectra(oracle, name, n)
    plain, weighted = _h0_errs(h0_np, h0)
    print(f"{name} N = {n}: {plain:.2e} plain, {weighted:.2e} weighted by |k|")
    assert plain <= H0_TOL and weighted <= 10 * H0_TOL, (plain, weighted)


@pytest.mark.parametrize("name,n", PAIRS)
def test_references_agree_on_prepared_spectra_at_t1(oracle, name, n):
    """prepareFFT of both references on the oracle's h0 at t = 1: measured <= 4.7e-7."""
    h0, _ = _spectra(oracle, name, n)
    s = oracle.default_settings(time=1.0, **SC.settings(name, n))
    hr, dr = oracle.prepare_fft(s, n, h0)
    hn, dn = R.prepare_fft(s, n, h0)
    err = max(lane_err(hn, hr) + lane_err(dn, dr))
    print(f"{name} N = {n}: {err:.2e}")
    assert err <= 1e-6, err


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _oracle_frames(oracle, name, n, steps, update=False, seed=None):
    """The OracleGenerator after `steps` at the case's settings (shared; read only)."""
    def make():
        kw = SC.settings(name, n)
        if seed is not None:
            kw["seed"] = seed
        ref = oracle.OracleGenerator(n, oracle.default_settings(**kw))
        for dt in steps:
            ref.calculate_ocean(dt, update_ocean=update)
        return ref

    return _shared(("frames", name, n, tuple(steps), update, seed), make)


def _maps(gen, c=0):
    return gen.height_map_host(c), gen.displacement_map_host(c), gen.jacobian_map_host(c)


def _print_frame_errs(tag, h, d, j, o):
    h64, d64, j64 = _f64_frame(o)
    print(tag, "vs oracle", " ".join(f"{e:.2e}" for e in channel_err(h, o.height) + channel_err(d, o.disp)),
          "| vs float64", " ".join(f"{e:.2e}" for e in channel_err(h, h64) + channel_err(d, d64)),
          f"| jacobian {scalar_err(j - 1.0, o.jac - 1.0):.2e} {scalar_err(j - 1.0, j64 - 1.0):.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_h0_at_case_settings(ocean, oracle, name, n):
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), **SC.settings(name, n))
    gen.GenerateSpectrum()
    got = gen.initial_spectrum_host(0)
    assert np.isfinite(got).all()
    plain, weighted = _h0_errs(got, _spectra(oracle, name, n)[0])
    print(f"h0 {name} N = {n}: {plain:.2e} plain, {weighted:.2e} weighted by |k|")
    assert plain <= H0_TOL and weighted <= 10 * H0_TOL, (plain, weighted)


@pytest.mark.gpu
@pytest.mark.parametrize("n,half", [(64, False), (1024, True), (1024, False)])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_frames_small_t(ocean, oracle, name, n, half):
    """Two frames (t = 1 + 1/60) on the full-spectrum path (N = 64, and 1024 with the switch off) and on the
    half-spectrum whole-grid launch (1024). The half path starts at N = 1024; the request at 64 is an error
    (test_half_spectrum_request_is_an_error_at_64)."""
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    gen.set_half_spectrum(half)
    ocean.apply_settings(gen.GetOceanSettings(0), **SC.settings(name, n))
    for dt in SMALL_T:
        gen.CalculateOcean(dt)
    ref = _oracle_frames(oracle, name, n, SMALL_T)
    assert gen.GetOceanSettings(0).time == ref.settings.time
    h, d, j = _maps(gen)
    _print_frame_errs(f"frames {name} N = {n} half = {half}:", h, d, j, ref)
    _frame_check(h, d, j, ref)


@pytest.mark.gpu
def test_half_spectrum_request_is_an_error_at_64(ocean):
    """Below N = 1024 there is no half-spectrum kernel: asking for one fails loudly and leaves the
    full-spectrum path selected (no quiet substitution either way)."""
    from oceansimulation_amd.capi import OceanError

    gen = ocean.Generator(ocean.FFTCalculator(64), 1)
    with pytest.raises(OceanError, match="1024"):
        gen.set_half_spectrum(True)
    assert gen.frame_bytes()[0] == 48.0  # the full-spectrum column pass's traffic


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shallow", "peak_shallow"])
def test_finite_depth_frame_at_t100(ocean, oracle, name):
    """One frame at t = 100, N = 64, where the phase noise between the references is visible. D is the
    disagreement of the references' prepared spectra at these settings and time (lane_err, worst lane), measured
    here; the gate per channel against the float64 transform of the oracle's spectrum is FRAME_TOL_GPU + 4 D:
    the device's 1 - 2 / (1 + e^{2kh}) has an absolute error of a few ulp of 1, so up to ~4 ulp of w where tanh is
    small, against <= 1 ulp for libm. A wrong branch or coefficient gives >= 1e-2; ulp-level drift passes.

    Measured on an MI355X (profiles/settings_parity.md), worst of the eight channels:
      shallow       D = 1.29e-5, gate 6.16e-5, error 1.18e-5 (channels 5.9e-6 .. 1.2e-5), Jacobian 1.0e-5
      peak_shallow  D = 4.49e-5, gate 1.90e-4, error 5.88e-6 (channels 9.7e-7 .. 5.9e-6), Jacobian 5.3e-6
    so the device is as close to the oracle as numpy_ref is (shallow) or closer (peak_shallow): no more than
    the ulps of tanh times t.
    """
    n = 64
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), **SC.settings(name, n))
    gen.CalculateOcean(100.0)
    ref = _oracle_frames(oracle, name, n, (100.0,))
    assert gen.GetOceanSettings(0).time == ref.settings.time == 100.0
    hr, dr = oracle.prepare_fft(ref.settings, n, ref.h0)
    hn, dn = R.prepare_fft(ref.settings, n, ref.h0)
    D = max(lane_err(hn, hr) + lane_err(dn, dr))
    gate = FRAME_TOL_GPU + 4.0 * D
    h, d, j = _maps(gen)
    h64, d64, j64 = _f64_frame(ref)
    errs = channel_err(h, h64) + channel_err(d, d64)
    print(f"t = 100 {name}: D = {D:.2e}, gate {gate:.2e}, channels " + " ".join(f"{e:.2e}" for e in errs) +
          f", jacobian {scalar_err(j - 1.0, j64 - 1.0):.2e}")
    assert np.isfinite(h).all() and np.isfinite(d).all() and np.isfinite(j).all()
    assert max(errs) <= gate, (errs, gate)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["peak", "light_gravity"])
def test_deep_water_stays_exact_long_time(ocean, oracle, name):
    """An hour of simulated time with the peak inside the grid / another gravity: tanh = 1 on every texel
    (test_cases_reach_their_branches), so w is bit-identical to the oracle's and the error does not grow with t
    (test_calculate_ocean_long_time at the defaults)."""
    n = 64
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), **SC.settings(name, n))
    ref = oracle.OracleGenerator(n, oracle.default_settings(**SC.settings(name, n)))
    for dt in (600.0, 3000.0):
        gen.CalculateOcean(dt)
        ref.calculate_ocean(dt)
        assert gen.GetOceanSettings(0).time == ref.settings.time
        h, d, j = _maps(gen)
        _print_frame_errs(f"long time {name} t = {ref.settings.time}:", h, d, j, ref)
        _frame_check(h, d, j, ref)


@pytest.mark.gpu
def test_g_and_h_are_read_live_by_the_frame_not_by_h0(ocean, oracle):
    """g and h edited between frames without the update flag: the frame evolves the old h0 with the new
    dispersion (src/Generator.cpp:55-72); with the flag, h0 follows — the h0 memo compares g and h too."""
    n, edit = 64, dict(h=0.5, g=3.71)
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    ref = oracle.OracleGenerator(n)
    gen.CalculateOcean(1.0)
    ref.calculate_ocean(1.0)
    h0 = gen.initial_spectrum_host(0)
    ocean.apply_settings(gen.GetOceanSettings(0), **edit)
    ocean.apply_settings(ref.settings, **edit)
    gen.CalculateOcean(1.0 / 60.0)
    ref.calculate_ocean(1.0 / 60.0)
    assert np.array_equal(gen.initial_spectrum_host(0), h0)
    h, d, j = _maps(gen)
    _print_frame_errs("live g, h:", h, d, j, ref)
    _frame_check(h, d, j, ref)
    gen.CalculateOcean(1.0 / 60.0, update_ocean=True)
    new = oracle.generate_spectrum(oracle.default_settings(**edit), n)
    assert max(lane_err(h0, new)) >= 1e-2  # the two seedings are far apart ...
    err = max(lane_err(gen.initial_spectrum_host(0), new))
    print(f"live g, h: re-seeded h0 {err:.2e}")
    assert err <= H0_TOL, err  # ... and the image holds the new one


@pytest.mark.gpu
def test_fused_reseed_in_finite_depth_at_the_peak(ocean, oracle):
    """test_fused_reseed_frames at peak_shallow: the column pass evaluates h0 itself (memo off, N = 1024), so
    the seeding math runs inlined there with the peak and the finite-depth branches live."""
    n, name, steps = 1024, "peak_shallow", (0.4, 1.0 / 60.0)
    fft = ocean.FFTCalculator(n)
    fused, plain = ocean.Generator(fft, 1), ocean.Generator(fft, 1)
    fused.set_h0_memo(False)
    for g in (fused, plain):
        ocean.apply_settings(g.GetOceanSettings(0), **SC.settings(name, n))
    for dt in steps:
        fused.CalculateOcean(dt, update_ocean=True)
        plain.GenerateSpectrum()
        plain.CalculateOcean(dt)
    ref = _oracle_frames(oracle, name, n, steps, update=True)
    for get in ("height_map_host", "displacement_map_host"):
        errs = lane_err(getattr(fused, get)(0), getattr(plain, get)(0))
        print(f"fused re-seed against seeded frames, {get}: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= 1e-5, (get, errs)
    h, d, j = _maps(fused)
    _print_frame_errs("fused re-seed:", h, d, j, ref)
    _frame_check(h, d, j, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1024])
def test_mixed_batch(ocean, oracle, n):
    """Four cascades that differ in wind, fetch, depth, gravity, direction, plane and seed in one generator
    (N = 1024: the half-spectrum path): each passes against its own oracle and is bit-identical to the same
    cascade computed alone."""
    fft = ocean.FFTCalculator(n)
    batch = ocean.Generator(fft, len(MIXED))
    seeds = [(12342 + 4097 * c, 8934 + 31 * c) for c in range(len(MIXED))]
    for c, name in enumerate(MIXED):
        ocean.apply_settings(batch.GetOceanSettings(c), seed=seeds[c], **SC.settings(name, n))
    for dt in SMALL_T:
        batch.CalculateOcean(dt)
    for c, name in enumerate(MIXED):
        ref = _oracle_frames(oracle, name, n, SMALL_T, seed=seeds[c])
        h, d, j = _maps(batch, c)
        _print_frame_errs(f"mixed batch N = {n} cascade {c} ({name}):", h, d, j, ref)
        _frame_check(h, d, j, ref)
        one = ocean.Generator(fft, 1)
        ocean.apply_settings(one.GetOceanSettings(0), seed=seeds[c], **SC.settings(name, n))
        for dt in SMALL_T:
            one.CalculateOcean(dt)
        for got, want in zip((h, d, j), _maps(one)):
            assert np.array_equal(got, want), (c, name)
        one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["peak", "shallow", "peak_shallow"])
def test_rate_maps_at_case_settings(ocean, name):
    """The rate maps scale with w itself, so this bounds the device's finite-depth w to 1e-5 of a channel's max
    without a factor of t (rates_ref evaluates tanh in float64)."""
    gen = ocean.Generator(ocean.FFTCalculator(64), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), **SC.settings(name, 64))
    gen.CalculateOcean(1.0)
    gen.calculate_rates()
    errs = _rate_errs(gen)
    print(f"rates {name}: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs


@pytest.mark.gpu
def test_slabs_in_finite_depth_match_whole_grid(ocean):
    """test_slab_decomposition_matches_whole_grid at peak_shallow, N = 256 over 4 ranks: bit for bit."""
    n, steps = 256, [0.25, 1.0 / 60.0]
    kw = SC.settings("peak_shallow", n)
    h, d, j = _slab_run(ocean, n, 4, steps, kw)
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    gen.set_half_spectrum(False)  # what slabs below 1024 run
    ocean.apply_settings(gen.GetOceanSettings(0), **kw)
    for dt in steps:
        gen.CalculateOcean(dt)
    for got, want in zip((h, d, j), _maps(gen)):
        assert np.array_equal(got, want)
