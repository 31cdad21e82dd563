"""ocean_generator_calculate_rates and ocean_surface_velocity: the time derivative of the maps and the
velocity of water particles, against their contract restated in numpy (tests/rates_ref.py).

Scenes as in test_surface_query.py: WaveApp's three cascades (planes 5 / 17 / 101 m), N = 64, t = 1;
"calm" is the default settings, "steep" has displacement = 1 and scale = 2. The CPU tests pin the
references on central differences at t = 1 +- 2^-10 (times that are exact in fp32); the GPU tests compare the
kernels with the references, the sampler bit for bit.

Gates, from the references alone (no GPU number went into them):
  RATE_FD   3e-4   rate reference against the central difference of numpy_ref's maps, max |err| / max |fd|
                   per channel: worst of all eight channels over 64^2 x {5, 17, 101 m} and 128^2 x 40 m is
                   7.3e-5 (truncation at delta = 2^-8 gives 1.0e-3, fp32 noise at 2^-12 gives 2.2e-4); 4 x that
                   still catches a wrong sign, channel or omega at O(1).
  VEL_FD    0.15 calm, 0.25 steep   velocity reference against the central difference of the forward sample,
                   worst point over max |fd| per component: a sanity bound only (bilinear samples of gradient
                   channels are not the gradient of the bilinear sample at 64^2); measured (x, y, z) =
                   (0.061, 0.018, 0.072) calm, (0.121, 0.092, 0.098) steep; a sign or channel mix-up gives >= 1.
  FRAME_TOL_GPU 1e-5   the GPU's rate maps against the float64 transform of the reference's packed images
                   (tests/parity.py): the frame's own arithmetic chain and bar.
Measured on an MI355X (the tests print every figure): rate maps 2.2e-7 .. 9.3e-7 per channel at N = 64 (t = 1
and t = 1000), 2.1e-6 at 256, 4.3e-6 at 1024 after a fused re-seed; the central difference of the GPU's own
frames 3.1e-5 .. 8.1e-5 against gates of 9e-4 .. 8e-3 at N = 64, 3.2e-5 .. 3.4e-4 against 1.8e-3 .. 2.1e-2 at 8192.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import numpy_ref as R
import rates_ref
from parity import FRAME_TOL_GPU, channel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
STEEP = dict(displacement=1.0, scale=2.0)
DELTA = 2.0 ** -10
RATE_FD = 3e-4
VEL_FD = {"calm": 0.15, "steep": 0.25}


def _base_points():
    return np.random.default_rng(3).uniform(-150.0, 150.0, (8192, 2)).astype(np.float32)


def _fd_err(rate, plus, minus, delta=DELTA):
    """max |rate - fd| / max |fd| per channel, fd the central difference in float64."""
    fd = (plus.astype(np.float64) - minus.astype(np.float64)) / (2.0 * delta)
    return [float(np.max(np.abs(rate[..., ch] - fd[..., ch])) / np.max(np.abs(fd[..., ch]))) for ch in range(4)]


# ---- without a GPU ----------------------------------------------------------------------------
def test_rates_are_exported_and_reject_null_arguments():
    from oceansimulation_amd import capi

    L = capi.lib()
    for name in ("ocean_generator_calculate_rates", "ocean_generator_height_rate_map",
                 "ocean_generator_displacement_rate_map", "ocean_surface_velocity"):
        assert hasattr(L, name) and name in capi.SIGNATURES
    assert L.ocean_generator_calculate_rates(None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_generator_calculate_rates" in L.ocean_last_error()
    assert L.ocean_surface_velocity(None, None, 0, None, 0, None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_surface_velocity" in L.ocean_last_error()
    for name in ("ocean_generator_height_rate_map", "ocean_generator_displacement_rate_map"):
        assert not getattr(L, name)(None, 0)
        assert name.encode() in L.ocean_last_error()


def _numpy_scene(n, planes, t, **overrides):
    """[(settings dict at time t, h0)] of numpy_ref, one per plane."""
    import oceansimulation_amd as ocean

    out = []
    for plane in planes:
        s = R.settings_dict(ocean.default_settings(planeSize=plane, **overrides))
        out.append((dict(s, time=t), R.generate_spectrum(s, n)))
    return out


def _numpy_maps(s, n, h0, t):
    hp, dp = R.prepare_fft(dict(s, time=t), n, h0)
    return R.encode_ifft(hp), R.encode_ifft(dp)


@pytest.mark.parametrize("n,planes", [(64, PLANES), (128, (40.0,))])
def test_rate_reference_against_central_difference(n, planes):
    worst = 0.0
    for s, h0 in _numpy_scene(n, planes, 1.0):
        rh, rd = rates_ref.rate_maps(s, n, h0)
        hp, dp = _numpy_maps(s, n, h0, 1.0 + DELTA)
        hm, dm = _numpy_maps(s, n, h0, 1.0 - DELTA)
        errs = _fd_err(rh, hp, hm) + _fd_err(rd, dp, dm)
        print(f"N = {n}, plane {s['planeSize']} m: " + " ".join(f"{e:.2e}" for e in errs))
        worst = max(worst, max(errs))
    assert worst <= RATE_FD, worst


def _forward(cascades, xz):
    """The vertex stage V(p) in float32 (ocean_surface_sample's slots 0-2)."""
    z = [(np.zeros_like(h), np.zeros_like(d)) for h, d, _, _, _ in cascades]
    return rates_ref.surface_velocity(cascades, z, xz)[:, :3]


@pytest.mark.parametrize("scene", ["calm", "steep"])
def test_velocity_reference_against_central_difference(scene):
    n = 64
    over = STEEP if scene == "steep" else {}
    cas, casp, casm, rates = [], [], [], []
    for s, h0 in _numpy_scene(n, PLANES, 1.0, **over):
        for t, dst in ((1.0, cas), (1.0 + DELTA, casp), (1.0 - DELTA, casm)):
            h, d = _numpy_maps(s, n, h0, t)
            dst.append((h, d, None, s["planeSize"], s["displacement"]))
        rates.append(rates_ref.rate_maps(s, n, h0))
    b = _base_points()
    fd = (_forward(casp, b).astype(np.float64) - _forward(casm, b)) / (2.0 * DELTA)
    scale = np.max(np.abs(fd), axis=0)
    got = rates_ref.surface_velocity(cas, rates, b)
    assert np.array_equal(got[:, :3], _forward(cas, b)) and np.all(got[:, [3, 7]] == 0.0)
    err = np.max(np.abs(got[:, 4:7] - fd), axis=0) / scale
    flat = rates_ref.surface_velocity(cas, rates, b, chain=False)
    err_flat = np.max(np.abs(flat[:, 4:7] - fd), axis=0) / scale
    print(f"{scene}: (x, y, z) error over max |fd| {err}, without the chain terms {err_flat}")
    assert np.all(err <= VEL_FD[scene]), err
    if scene == "calm":
        assert err[1] < err_flat[1]


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _rate_errs(gen, cascade=0):
    """channel_err of both GPU rate maps of a cascade against the reference on the generator's own h0 and
    settings (time as accumulated)."""
    s = R.settings_dict(gen.GetOceanSettings(cascade))
    rh, rd = rates_ref.rate_maps(s, gen.n, gen.initial_spectrum_host(cascade))
    return channel_err(gen.height_rate_map_host(cascade), rh) + channel_err(gen.displacement_rate_map_host(cascade), rd)


@pytest.mark.gpu
@pytest.mark.parametrize("plane", PLANES)
def test_rate_maps_against_reference(ocean, plane):
    gen = ocean.Generator(ocean.FFTCalculator(64), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=plane)
    for step in (1.0, 999.0):  # t = 1, then t = 1000
        gen.CalculateOcean(step)
        gen.calculate_rates()
        errs = _rate_errs(gen)
        print(f"plane {plane} m, t = {gen.GetOceanSettings(0).time}: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= FRAME_TOL_GPU, errs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 32, 256])
def test_rate_maps_other_sizes(ocean, n):
    """The packing kernel's other shapes: h0 strips shorter than a tile (16: 1 column, 32: 2 columns; one tile
    per work item) and strips of several tiles (256)."""
    gen = ocean.Generator(ocean.FFTCalculator(n), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=17.0)
    gen.CalculateOcean(1.0)
    gen.calculate_rates()
    errs = _rate_errs(gen)
    print(f"N = {n}: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs


@pytest.mark.gpu
def test_rate_maps_half_spectrum_path_after_fused_reseed(ocean):
    """N = 1024: the half-spectrum path and its h0 strip width; the second frame re-seeds h0 inside the column
    pass (U_10 changed, so the memo cannot skip it) and leaves the h0 image stale for calculate_rates."""
    gen = ocean.Generator(ocean.FFTCalculator(1024), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=40.0)
    gen.CalculateOcean(0.5)
    gen.GetOceanSettings(0).U_10 = 25.0
    gen.CalculateOcean(0.5, True)
    gen.calculate_rates()
    errs = _rate_errs(gen)
    print("N = 1024 after a fused re-seed: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs
    # the h0 the rates were evolved from is the re-seeded one
    s = R.settings_dict(gen.GetOceanSettings(0))
    h0 = gen.initial_spectrum_host(0)
    new, old = R.generate_spectrum(s, 1024), R.generate_spectrum(dict(s, U_10=40.0), 1024)
    assert R.rel_err(old, new) >= 1e-2  # the two seedings are far apart (7 % of max |h0|) ...
    assert R.rel_err(h0, new) <= 1e-3   # ... and the image holds the new one


@pytest.mark.gpu
def test_rate_maps_two_column_h0_strips(ocean):
    """N = 2048, one cascade: the half-strip column pass keeps h0 in 2-column strips (k_rates_pack<true> with
    lcw = 3: a block is 8 columns x 128 rows), the default path of a one-cascade 2048^2 or 4096^2 ocean. Then the
    full-spectrum path: h0 goes back to 4-column strips, the same values, and the rates still pass."""
    from oceansimulation_amd import capi

    L = capi.lib()
    fft = ocean.FFTCalculator(2048)
    gen = ocean.Generator(fft, 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=401.0)
    gen.CalculateOcean(1.0)
    assert int(L.ocean_generator_spectrum_block(gen.handle)) == 2
    gen.calculate_rates()
    errs = _rate_errs(gen)
    print("N = 2048, 2-column strips: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs
    h0 = gen.initial_spectrum_host(0)
    assert h0.any()
    gen.set_half_spectrum(False)
    gen.CalculateOcean(1.0 / 60.0)
    assert int(L.ocean_generator_spectrum_block(gen.handle)) == 4
    gen.calculate_rates()
    errs = _rate_errs(gen)
    print("N = 2048, full spectrum, 4-column strips: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs
    assert np.array_equal(gen.initial_spectrum_host(0).view(np.uint32), h0.view(np.uint32))
    gen.close()
    fft.close()


@pytest.mark.gpu
def test_rate_maps_of_a_batched_generator(ocean):
    gen = ocean.Generator(ocean.FFTCalculator(64), 3)
    for c, plane in enumerate(PLANES):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=plane)
    gen.CalculateOcean(1.0)
    gen.calculate_rates()
    for c in range(3):
        errs = _rate_errs(gen, c)
        print(f"cascade {c}: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= FRAME_TOL_GPU, errs


@pytest.mark.gpu
@pytest.mark.parametrize("plane", PLANES)
def test_rates_are_the_derivative_of_the_frames(ocean, plane):
    """The central difference of the GPU's own maps at t = 1 -+ 2^-10 against the rates at t = 1. Gate per
    channel: RATE_FD plus the maps' own fp32 error (FRAME_TOL_GPU of a channel's max) through the difference."""
    gen = ocean.Generator(ocean.FFTCalculator(64), 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=plane)
    gen.CalculateOcean(1.0 - DELTA)
    minus = np.concatenate([gen.height_map_host(0), gen.displacement_map_host(0)], -1)
    gen.CalculateOcean(DELTA)
    assert gen.GetOceanSettings(0).time == 1.0
    gen.calculate_rates()
    rate = np.concatenate([gen.height_rate_map_host(0), gen.displacement_rate_map_host(0)], -1)
    gen.CalculateOcean(DELTA)
    plus = np.concatenate([gen.height_map_host(0), gen.displacement_map_host(0)], -1)
    fd = (plus.astype(np.float64) - minus) / (2.0 * DELTA)
    for ch in range(8):
        err = float(np.max(np.abs(rate[..., ch] - fd[..., ch])) / np.max(np.abs(fd[..., ch])))
        gate = RATE_FD + FRAME_TOL_GPU * float(np.max(np.abs(plus[..., ch]))) / (DELTA * float(np.max(np.abs(rate[..., ch]))))
        print(f"plane {plane} m, channel {ch}: {err:.2e} (gate {gate:.2e})")
        assert err <= gate, (ch, err, gate)


class _DevicePtr:
    """A device buffer of the library seen by torch (no copy)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


@pytest.mark.gpu
def test_rates_are_the_derivative_of_the_frames_8192(ocean):
    """The four-step frame path's h0 layout (64-column strips) and a map of 1 GiB: the same end-to-end check
    with the differences taken on the device. Plane 4093 m: the fastest wave has w = 7.9 rad/s, below the
    20 rad/s of N = 64 on 5 m, so the central difference truncates no more than there and the gate is the same."""
    import torch

    from oceansimulation_amd import capi

    n = 8192
    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, 1)
    assert int(capi.lib().ocean_generator_spectrum_block(gen.handle)) == 64
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=4093.0)
    maps = torch.as_tensor(_DevicePtr(gen.GetHeightMap(0), (2, n, n, 4)), device="cuda")  # heightMap, displacementMap
    gen.CalculateOcean(1.0 - DELTA)
    fft.synchronize()
    minus = maps.clone()
    torch.cuda.synchronize()
    gen.CalculateOcean(DELTA)
    gen.calculate_rates()
    gen.CalculateOcean(DELTA)
    fft.synchronize()
    rate = torch.as_tensor(_DevicePtr(capi.lib().ocean_generator_height_rate_map(gen.handle, 0), (2, n, n, 4)), device="cuda")
    fd = (maps.double() - minus.double()) / (2.0 * DELTA)
    err = ((rate.double() - fd).abs().amax(dim=(1, 2)) / fd.abs().amax(dim=(1, 2))).reshape(8).cpu().numpy()
    gate = (RATE_FD + FRAME_TOL_GPU * maps.abs().amax(dim=(1, 2)).double() / (DELTA * rate.abs().amax(dim=(1, 2)).double()))
    gate = gate.reshape(8).cpu().numpy()
    print("N = 8192: " + " ".join(f"{e:.2e} ({g:.2e})" for e, g in zip(err, gate)))
    assert np.all(err <= gate), (err, gate)
    del maps, minus, rate, fd
    torch.cuda.empty_cache()


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


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["calm", "steep"])
def test_velocity_bit_exact(ocean, calm64, scene):
    sampler, host, rates = calm64 if scene == "calm" else _scene(ocean, 64, **STEEP)
    b = _base_points()
    got = sampler.velocity_host(b)
    want = rates_ref.surface_velocity(host, rates, b)
    assert np.array_equal(got, want), np.max(np.abs(got - want))
    assert np.array_equal(got[:, :3], sampler.sample_host(b)[:, :3])
    assert np.all(got[:, [3, 7]] == 0.0)
    print(f"{scene}: max speed {np.sqrt((got[:, 4:7].astype(np.float64) ** 2).sum(1)).max():.3f} m/s")


@pytest.mark.gpu
def test_velocity_after_a_query_filled_the_atlas_and_no_points(ocean, calm64):
    """70000 points: the query before it samples the plan's repacked atlas; the velocity sampler reads the
    maps themselves and still matches."""
    sampler, host, rates = calm64
    q = np.random.default_rng(11).uniform(-400.0, 400.0, (70000, 2)).astype(np.float32)
    sampler.query_host(q, 8, 0.0)
    assert np.array_equal(sampler.velocity_host(q), rates_ref.surface_velocity(host, rates, q))
    assert sampler.velocity_host(np.zeros((0, 2), np.float32)).shape == (0, 8)


@pytest.mark.gpu
def test_rates_and_velocity_fail_loudly(ocean):
    from oceansimulation_amd import capi
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.slab import SlabGenerator
    from oceansimulation_amd.surface import SurfaceSampler

    L = capi.lib()
    fft = ocean.FFTCalculator(64)
    gens = [ocean.Generator(fft, 1) for _ in range(2)]
    q = np.zeros((4, 2), np.float32)
    with pytest.raises(OceanError, match="no frame"):  # rates before any frame
        gens[0].calculate_rates()
    assert not L.ocean_generator_height_rate_map(gens[0].handle, 0)  # getters before the first calculate_rates
    assert b"never calculated" in L.ocean_last_error()
    assert not L.ocean_generator_displacement_rate_map(gens[0].handle, 0)
    with pytest.raises(OceanError):
        gens[0].height_rate_map_host(0)
    slab = SlabGenerator(ocean.FFTCalculator(256), 0, 2)
    assert L.ocean_generator_calculate_rates(slab.handle) == capi.OCEAN_ERR_INVALID  # rates on a slab generator
    assert b"slab" in L.ocean_last_error()
    for g in gens:
        g.CalculateOcean(1.0)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    gens[0].calculate_rates()
    with pytest.raises(OceanError, match="generator 1 has no rates"):  # rates never calculated
        sampler.velocity_host(q)
    gens[1].calculate_rates()
    assert sampler.velocity_host(q).shape == (4, 8)
    assert L.ocean_generator_height_rate_map(gens[1].handle, 0) and not L.ocean_generator_height_rate_map(gens[1].handle, 1)
    gens[1].CalculateOcean(0.25)
    with pytest.raises(OceanError, match="generator 1 has stale rates"):  # stale after a further frame
        sampler.velocity_host(q)
    gens[1].calculate_rates()
    assert sampler.velocity_host(q).shape == (4, 8)
    other = ocean.Generator(ocean.FFTCalculator(128), 1)
    other.CalculateOcean(1.0)
    other.calculate_rates()
    with pytest.raises(OceanError, match="one map size"):  # mixed map sizes
        SurfaceSampler([(gens[0], 0), (other, 0)]).velocity_host(q)


@pytest.mark.gpu
def test_waveapp_headless_velocity(ocean, tmp_path):
    """--velocity: the velocities at the probes' base points equal the reference on the dumped maps and rate maps."""
    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "4", "--mesh", "0", "--probes", "64", "--velocity", "--dump",
                        str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    scene = json.load(open(tmp_path / "scene.json"))
    cas = [(np.load(tmp_path / f"height_{i}.npy"), np.load(tmp_path / f"disp_{i}.npy"), np.load(tmp_path / f"jac_{i}.npy"),
            c["planeSize"], c["displacement"]) for i, c in enumerate(scene["cascades"])]
    rates = [(np.load(tmp_path / f"height_rate_{i}.npy"), np.load(tmp_path / f"disp_rate_{i}.npy")) for i in range(3)]
    base = np.load(tmp_path / "probes.npy")[:, [0, 2]]
    got = np.load(tmp_path / "probe_velocity.npy")
    assert got.shape == (64, 8) and rates[0][0].shape == (64, 64, 4)
    assert np.array_equal(got, rates_ref.surface_velocity(cas, rates, base))
    u = got[:, 4:7]
    speed = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]).max()
    assert np.float32(out["probe_max_speed"]) == speed and speed > 0.0
    # without the flag nothing changes
    r = subprocess.run([exe, "--n", "64", "--frames", "2", "--mesh", "0", "--probes", "8"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "probe_max_speed" not in r.stdout
