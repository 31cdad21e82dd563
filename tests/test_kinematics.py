"""Depth layers (ocean_generator_set_depth_layers / _calculate_kinematics / _kinematics_map) and the sampler
ocean_water_kinematics, against their contract restated in numpy (tests/kinematics_ref.py).

Scene as in test_rates.py: WaveApp's three cascades (planes 5 / 17 / 101 m), t = 1, depths (0, 0.25, 1, 4) m
unless stated; "calm" is the default settings, "steep" has displacement = 1 and scale = 2. The CPU tests pin
the references on each other; the GPU tests compare the kernels with the references, the sampler bit for bit.

Gates:
  RATE_FD   3e-4   test_rates.py's gate, derived there from the references alone (worst 7.3e-5 unattenuated). The
                   attenuated lanes at depths 0.25 and 1 m measure 1.6e-5 .. 5.6e-5 on the CPU (six channels, 64^2 x
                   {5, 17, 101 m}; the factors weaken the fast waves that dominate the truncation), so the worst
                   case does not move and the gate stays.
  FRAME_TOL_GPU 1e-5   the GPU's layer maps against the float64 transform of the reference's packed images
                   (tests/parity.py): the frame's own bar, on the six named channels.
  Layer 0 against the GPU's own rate maps, and the sampler against the restatement on the GPU's own maps: bit
  for bit, no tolerance.
Measured on an MI355X (the tests print every figure), worst of the six channels over cascades and layers: 7.8e-7,
1.7e-6, 2.1e-6, 2.6e-6 at N = 16, 32, 64, 256; 4.3e-6 at 1024 after a fused re-seed; 9.4e-7 (h = 0.2), 9.1e-7 (h = 1),
1.9e-6 (g = 3.71), 1.8e-6 (t = 1000). Layer 0 equalled the rate maps bit for bit at N = 64 and 8192.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kinematics_ref as K
import numpy_ref as R
import rates_ref
from parity import FRAME_TOL_GPU, channel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
DEPTHS = (0.0, 0.25, 1.0, 4.0)
STEEP = dict(displacement=1.0, scale=2.0)
DELTA = 2.0 ** -10
RATE_FD = 3e-4
NAMED = ((0, 0), (0, 1), (0, 3), (1, 0), (1, 2), (1, 3))  # (image, channel): w, dw/dx, dDx/dt, dDz/dt, P, dP/dx
BELOW = (-1.0, 0.1, 0.5, 2.0, 10.0)  # eta - Y of the sampler's test points
NEW_CALLS = ("ocean_generator_set_depth_layers", "ocean_generator_depth_layers", "ocean_generator_calculate_kinematics",
             "ocean_generator_kinematics_map", "ocean_water_kinematics")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


# ---- without a GPU ----------------------------------------------------------------------------
def test_exports_and_signatures():
    from oceansimulation_amd import capi
    import oceansimulation_amd as ocean
    from oceansimulation_amd.surface import SurfaceSampler

    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    for name in ("set_depth_layers", "depth_layers", "calculate_kinematics", "kinematics_map_host", "GetKinematicsMap"):
        assert hasattr(ocean.Generator, name), name
    assert hasattr(SurfaceSampler, "kinematics") and hasattr(SurfaceSampler, "kinematics_host")


def test_rejected_arguments_name_the_call():
    """Everything that can be refused without a generator: OCEAN_ERR_INVALID (or a null pointer, or a count of
    0) with the entry point's name in ocean_last_error."""
    from oceansimulation_amd import capi

    L = capi.lib()
    inv = capi.OCEAN_ERR_INVALID
    assert L.ocean_generator_set_depth_layers(None, _floats(DEPTHS), 4) == inv
    assert b"ocean_generator_set_depth_layers: null generator" in L.ocean_last_error()
    assert L.ocean_generator_calculate_kinematics(None) == inv
    assert b"ocean_generator_calculate_kinematics: null generator" in L.ocean_last_error()
    assert not L.ocean_generator_kinematics_map(None, 0, 0, 0)
    assert b"ocean_generator_kinematics_map" in L.ocean_last_error()
    assert L.ocean_generator_depth_layers(None, None) == 0
    one = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
    g1, c1 = (ctypes.c_void_p * 1)(None), (ctypes.c_int * 1)(0)
    g17, c17 = (ctypes.c_void_p * 17)(*([16] * 17)), (ctypes.c_int * 17)()
    for args, word in (((None, c1, 1), b"pairs"), ((g1, None, 1), b"pairs"), ((g1, c1, 0), b"pairs"),
                       ((g17, c17, 17), b"pairs"), ((g1, c1, 1), b"null generator")):
        assert L.ocean_water_kinematics(*args, one, ctypes.c_int64(4), 8, ctypes.c_float(0.0), one) == inv, word
        assert b"ocean_water_kinematics:" in L.ocean_last_error() and word in L.ocean_last_error(), L.ocean_last_error()


@pytest.mark.parametrize("depths,word", [
    ((0.0, 1.0, 0.5), b"ascending"),            # unsorted
    ((0.0, 1.0, 1.0), b"ascending"),            # not strictly
    ((-0.5, 1.0), b">= 0"),                     # negative
    ((0.0, float("nan")), b"finite"),
    ((0.0, float("inf")), b"finite"),
    ((), b"1..8"),                              # empty
    (tuple(float(i) for i in range(9)), b"1..8"),  # longer than 8
])
def test_bad_depth_lists_are_refused(depths, word):
    """The list's rules are checked before the generator, so they are refused here without a device."""
    from oceansimulation_amd import capi

    L = capi.lib()
    arr = _floats(depths) if depths else _floats((0.0,))
    assert L.ocean_generator_set_depth_layers(None, arr, len(depths)) == capi.OCEAN_ERR_INVALID
    msg = L.ocean_last_error()
    assert b"ocean_generator_set_depth_layers:" in msg and word in msg and b"null generator" not in msg, msg
    assert L.ocean_generator_set_depth_layers(None, None, 2) == capi.OCEAN_ERR_INVALID
    assert b"1..8" in L.ocean_last_error()


def test_cpp_headers_compile_standalone(tmp_path):
    """A consumer of the depth layers compiles against the drop-in headers alone."""
    src = tmp_path / "consumer.cpp"
    src.write_text(
        '#include "waves/Surface.h"\n'
        "#include <vector>\n"
        "Vision::ID frame(Waves::SurfaceSampler& s, std::vector<Waves::Generator*>& gens, float dt, const float* xyz) {\n"
        "  const float depths[4] = {0.0f, 0.25f, 1.0f, 4.0f};\n"
        "  float back[8];\n"
        "  for (auto* g : gens) {\n"
        "    g->SetDepthLayers(depths, 4);\n"
        "    g->CalculateOcean(dt); g->CalculateKinematics();\n"
        "    Vision::ID w = g->GetKinematicsMap(3, 1); (void)w;\n"
        "    if (g->GetDepthLayers(back) != 4) return 0;\n"
        "  }\n"
        "  return s.Kinematics(gens, xyz, 64, 8, 0.0f);\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}/include", "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    so = os.path.join(ROOT, "oceansimulation_amd", "libwaves.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", so], capture_output=True, text=True).stdout
    for sig in ("Waves::Generator::SetDepthLayers(float const*, int)", "Waves::Generator::CalculateKinematics()",
                "Waves::Generator::GetKinematicsMap(int, int) const", "Waves::SurfaceSampler::Kinematics("):
        assert sig in syms, sig


def _numpy_scene(n, planes, t, **overrides):
    """[(settings dict at time t, h0)] of numpy_ref, one per plane."""
    import oceansimulation_amd as ocean

    out = []
    for plane in planes:
        s = R.settings_dict(ocean.default_settings(planeSize=plane, **overrides))
        out.append((dict(s, time=t), R.generate_spectrum(s, n)))
    return out


@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("h", [100.0, 1.0, 0.2])
def test_reference_layer_zero_is_the_surface(n, h):
    """At d = 0 both factors are exactly 1: the four lanes are the rate maps' and the height map's, bit for bit."""
    for s, h0 in _numpy_scene(n, PLANES, 1.0, h=h):
        (i0, i1), = K.layer_maps(s, n, h0, (0.0,))
        rh, rd = rates_ref.rate_maps(s, n, h0)
        hm = R.encode_ifft(K.prepare_height(s, n, h0))
        assert np.array_equal(_bits(i0[..., 0:2]), _bits(rh[..., 0:2])), (s["planeSize"], "image 0 xy")
        assert np.array_equal(_bits(i0[..., 2:4]), _bits(rh[..., 2:4])), (s["planeSize"], "image 0 zw")
        assert np.array_equal(_bits(i1[..., 0:2]), _bits(rd[..., 0:2])), (s["planeSize"], "image 1 xy")
        assert np.array_equal(_bits(i1[..., 2:4]), _bits(hm[..., 0:2])), (s["planeSize"], "image 1 zw")
        # prepare_height is numpy_ref.prepare_fft's height image: the same bits wherever the two float32
        # dispersions agree (everywhere but a few of the longest waves, where numpy's float32 tanh is an ulp
        # off), and the same height map within fp32 rounding at t = 1
        mine, theirs = K.prepare_height(s, n, h0), R.prepare_fft(s, n, h0)[0]
        k = K.wavenumbers(s, n)
        same_w = rates_ref._dispersion(k, np.float32(s["g"]), np.float32(s["h"])) == R._dispersion(
            k, np.float32(s["g"]), np.float32(s["h"]))
        assert np.array_equal(_bits(mine[same_w]), _bits(theirs[same_w])) and same_w.mean() >= 0.5, (s["planeSize"], same_w.mean())
        assert max(channel_err(hm, R.encode_ifft(theirs))) <= 1e-6, s["planeSize"]


@pytest.mark.parametrize("h", [0.2, 1.0])
def test_reference_no_vertical_velocity_at_the_bed(h):
    n = 64
    for s, h0 in _numpy_scene(n, PLANES, 1.0, h=h):
        for d, (i0, _) in zip(DEPTHS, K.layer_maps(s, n, h0, DEPTHS)):
            if d >= h:
                assert not i0[..., 0].any() and not i0[..., 1].any(), (s["planeSize"], d)
            else:
                assert i0[..., 0].any(), (s["planeSize"], d)
    ah, av = K.attenuation(np.float32([0.0621, 1.26, 80.0]), 0.5, 0.0)  # h == 0: no vertical motion at all
    assert not av.any() and np.all(ah == 1.0)


def test_reference_channels_decay_with_depth():
    n = 64
    for s, h0 in _numpy_scene(n, PLANES, 1.0):
        norms = np.array([[np.max(np.abs(maps[i][..., ch])) for i, ch in NAMED] for maps in K.layer_maps(s, n, h0, DEPTHS)])
        print(f"plane {s['planeSize']} m, max |channel| per depth:\n{norms}")
        assert np.all(norms[1:] < norms[:-1]), s["planeSize"]
    ah, av = K.attenuation(np.float32([1.26]), 1.0, 100.0)  # the 5 m cascade loses more than a factor of 10 over 1 m
    assert ah[0] < 0.3 and abs(ah[0] - np.exp(-1.26)) < 1e-6 and abs(av[0] - ah[0]) < 1e-6


def _attenuated_h_maps(s, n, h0, t, d):
    """The transforms of the H lanes at time t, attenuated as the layer's Hd lanes are: image 0's counterpart
    (A_v * lane xy, A_h * lane zw of the height packing) and image 1's lane xy (A_h * lane xy of the displacement
    packing; the other lane is zero)."""
    sd = dict(s, time=t)
    ah, av = K.attenuation(K.wavenumbers(sd, n), d, sd["h"])
    hp, dp = R.prepare_fft(sd, n, h0)
    dp = dp.copy()
    dp[..., 2:4] = 0
    return R.encode_ifft(K.scale_lanes(hp, av, ah)), R.encode_ifft(K.scale_lanes(dp, ah, ah))


@pytest.mark.parametrize("d", [0.25, 1.0])
def test_reference_layers_against_central_difference(d):
    """The Hd lanes of a layer are the time derivative of the H lanes attenuated the same way: six channels
    (image 0's four, image 1's .x and .y) against the central difference at t = 1 +- 2^-10."""
    n, worst = 64, 0.0
    for s, h0 in _numpy_scene(n, PLANES, 1.0):
        (i0, i1), = K.layer_maps(s, n, h0, (d,))
        p0, p1 = _attenuated_h_maps(s, n, h0, 1.0 + DELTA, d)
        m0, m1 = _attenuated_h_maps(s, n, h0, 1.0 - DELTA, d)
        errs = []
        for rate, plus, minus, chans in ((i0, p0, m0, range(4)), (i1, p1, m1, range(2))):
            fd = (plus.astype(np.float64) - minus.astype(np.float64)) / (2.0 * DELTA)
            errs += [float(np.max(np.abs(rate[..., ch] - fd[..., ch])) / np.max(np.abs(fd[..., ch]))) for ch in chans]
        print(f"depth {d} m, plane {s['planeSize']} m: " + " ".join(f"{e:.2e}" for e in errs))
        worst = max(worst, max(errs))
    assert worst <= RATE_FD, worst


def _test_points(eta_of, count=8192, seed=3):
    """World positions whose depth under the surface cycles through BELOW: (xyz, the delta of each point)."""
    xz = np.random.default_rng(seed).uniform(-150.0, 150.0, (count, 2)).astype(np.float32)
    eta = eta_of(xz)
    delta = np.float32(BELOW)[np.arange(count) % len(BELOW)]
    return np.stack([xz[:, 0], (eta - delta).astype(np.float32), xz[:, 1]], 1), delta


def _branches_populated(out, delta, depths=DEPTHS):
    """Every branch of the layer choice is taken by the test points: above the water, between each pair of layers,
    below the last."""
    l, f, wet = out[:, 9], out[:, 10], out[:, 11]
    above = delta < 0
    assert above.any() and np.all(wet[above] == 0) and np.all(l[above] == 0) and np.all(f[above] == 0)
    assert np.all(out[above, 8] == 0) and np.all(wet[~above] == 1)
    for j in range(len(depths) - 1):
        between = (delta > depths[j]) & (delta < depths[j + 1])
        assert between.any() and np.all(l[between] == j) and np.all((f[between] > 0) & (f[between] < 1)), j
    below = delta > depths[-1]
    assert below.any() and np.all(l[below] == len(depths) - 1) and np.all(f[below] == 0)


@pytest.mark.parametrize("scene", ["calm", "steep"])
def test_reference_sampler(oracle, scene):
    from surface_query_ref import surface_query

    n = 64
    cas, rates, layers = [], [], []
    for s, h0 in _numpy_scene(n, PLANES, 1.0, **(STEEP if scene == "steep" else {})):
        hp, dp = R.prepare_fft(s, n, h0)
        hm, dm = R.encode_ifft(hp), R.encode_ifft(dp)
        cas.append((hm, dm, R.compute_foam(s, dm), s["planeSize"], s["displacement"]))
        rates.append(rates_ref.rate_maps(s, n, h0))
        layers.append(K.layer_maps(s, n, h0, DEPTHS))
    xyz, delta = _test_points(lambda xz: surface_query(oracle, cas, xz, 8, 0.0)[:, 1])
    out = K.water_kinematics(oracle, cas, layers, DEPTHS, xyz, 8, 0.0)
    _branches_populated(out, delta)
    q = surface_query(oracle, cas, xyz[:, [0, 2]], 8, 0.0)
    assert np.array_equal(_bits(out[:, :4]), _bits(q[:, [0, 1, 2, 7]]))
    # at or above the water: the surface particle's velocity without the chain terms, bit for bit
    above = delta < 0
    flat = rates_ref.surface_velocity(cas, rates, q[:, [0, 2]], chain=False)
    assert np.array_equal(_bits(out[above, 4:7]), _bits(flat[above, 4:7]))
    # under water the speed falls with depth (the mean over the points of each depth)
    speed = np.sqrt((out[:, 4:7].astype(np.float64) ** 2).sum(1))
    means = [speed[delta == np.float32(b)].mean() for b in BELOW[1:]]
    print(f"{scene}: mean speed at {BELOW[1:]} m under the surface: {means}")
    assert all(a > b for a, b in zip(means, means[1:]))
    # a NaN height is dry and samples layer 0
    l, f = K.choose_layer(np.float32([np.nan, 0.0, 0.25, 4.0, 5.0]), DEPTHS)
    assert list(l) == [0, 0, 1, 3, 3] and not f.any()


# ---- on the GPU -------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _layer_errs(gen, cascade, depths):
    """channel_err of the six named channels of every layer of a cascade against the reference on the generator's
    own h0 and settings (time as accumulated): [layer][6]."""
    s = R.settings_dict(gen.GetOceanSettings(cascade))
    want = K.layer_maps(s, gen.n, gen.initial_spectrum_host(cascade), depths)
    errs = []
    for layer in range(len(depths)):
        got = [gen.kinematics_map_host(cascade, layer, image) for image in range(2)]
        per_image = [channel_err(got[image], want[layer][image]) for image in range(2)]
        errs.append([per_image[i][ch] for i, ch in NAMED])
    return errs


def _check_layers(gen, depths, label):
    for c in range(gen.cascades):
        for layer, errs in enumerate(_layer_errs(gen, c, depths)):
            print(f"{label}, cascade {c}, depth {depths[layer]} m: " + " ".join(f"{e:.2e}" for e in errs))
            assert max(errs) <= FRAME_TOL_GPU, (label, c, layer, errs)


@gpu
@pytest.mark.parametrize("n", [16, 32, 64, 256])
def test_layer_maps_against_reference(ocean, n):
    """The packing kernel's linear shape (16, 32) and its block shape (64, 256), three cascades."""
    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, 3)
    for c, plane in enumerate(PLANES):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=plane)
    gen.set_depth_layers(DEPTHS)
    assert np.array_equal(gen.depth_layers(), np.float32(DEPTHS))
    gen.CalculateOcean(1.0)
    gen.calculate_kinematics()
    _check_layers(gen, DEPTHS, f"N = {n}")
    gen.close()
    fft.close()


@gpu
def test_layer_maps_half_spectrum_path_after_fused_reseed(ocean):
    """N = 1024, one cascade: the half-spectrum path's h0 strip width, the h0 image left stale by a fused re-seed."""
    fft = ocean.FFTCalculator(1024)
    gen = ocean.Generator(fft, 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=40.0)
    gen.set_depth_layers(DEPTHS)
    gen.CalculateOcean(0.5)
    gen.GetOceanSettings(0).U_10 = 25.0
    gen.CalculateOcean(0.5, True)
    gen.calculate_kinematics()
    _check_layers(gen, DEPTHS, "N = 1024 after a fused re-seed")
    gen.close()
    fft.close()


@gpu
@pytest.mark.parametrize("case", ["h=0.2", "h=1", "g=3.71", "t=1000"])
def test_layer_maps_settings(ocean, case):
    over = {"h=0.2": dict(h=0.2), "h=1": dict(h=1.0), "g=3.71": dict(g=3.71), "t=1000": {}}[case]
    fft = ocean.FFTCalculator(64)
    gen = ocean.Generator(fft, 3)
    for c, plane in enumerate(PLANES):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=plane, **over)
    gen.set_depth_layers(DEPTHS)
    gen.CalculateOcean(1000.0 if case == "t=1000" else 1.0)
    gen.calculate_kinematics()
    _check_layers(gen, DEPTHS, case)
    if case in ("h=0.2", "h=1"):  # no vertical velocity at or below the bed, exactly
        for c in range(3):
            for layer, d in enumerate(DEPTHS):
                if d >= over["h"]:
                    w = gen.kinematics_map_host(c, layer, 0)
                    assert not w[..., 0].any() and not w[..., 1].any(), (c, d)
    gen.close()
    fft.close()


@gpu
def test_layer_zero_is_the_rate_maps_bit_for_bit(ocean):
    """The factor is 1.0f and EncodeIFFT's two lanes are independent: image 0 .x / .w and image 1 .x of layer 0
    are the rate maps' dh/dt, dDx/dt and dDz/dt, and image 1 .z is the height map's h."""
    fft = ocean.FFTCalculator(64)
    gen = ocean.Generator(fft, 3)
    for c, plane in enumerate(PLANES):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=plane)
    gen.set_depth_layers(DEPTHS)
    gen.CalculateOcean(1.0)
    gen.calculate_rates()
    gen.calculate_kinematics()
    for c in range(3):
        i0, i1 = gen.kinematics_map_host(c, 0, 0), gen.kinematics_map_host(c, 0, 1)
        rh, rd, hm = gen.height_rate_map_host(c), gen.displacement_rate_map_host(c), gen.height_map_host(c)
        assert np.array_equal(_bits(i0[..., 0]), _bits(rh[..., 0])), c
        assert np.array_equal(_bits(i0[..., 3]), _bits(rh[..., 3])), c
        assert np.array_equal(_bits(i1[..., 0]), _bits(rd[..., 0])), c
        print(f"cascade {c}: image 0 .y / .z against the rate map's: "
              f"{np.array_equal(_bits(i0[..., 1:3]), _bits(rh[..., 1:3]))}, image 1 .z against h: "
              f"{channel_err(i1[..., 2:3], hm[..., 0:1])[0]:.2e}")
    gen.close()
    fft.close()


@gpu
def test_layers_two_column_h0_strips(ocean):
    """N = 2048, one cascade, layers (0, 1 m): k_kinematics_pack<true> on the 2-column h0 strips of the half-strip
    column pass (lcw = 3: a block is 8 columns x 128 rows). Layer 0 is the rate maps bit for bit, and image 1 .z
    the height map's h as far as test_layer_zero_is_the_rate_maps_bit_for_bit holds it (the frame and EncodeIFFT
    transform one spectrum with different kernels: within twice the frame's gate, and the test prints whether the
    bits agree); layer 1 against the reference."""
    from oceansimulation_amd import capi

    depths = (0.0, 1.0)
    fft = ocean.FFTCalculator(2048)
    gen = ocean.Generator(fft, 1)
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=401.0)
    gen.set_depth_layers(depths)
    gen.CalculateOcean(1.0)
    assert int(capi.lib().ocean_generator_spectrum_block(gen.handle)) == 2
    gen.calculate_rates()
    gen.calculate_kinematics()
    i0, i1 = gen.kinematics_map_host(0, 0, 0), gen.kinematics_map_host(0, 0, 1)
    rh, rd, hm = gen.height_rate_map_host(0), gen.displacement_rate_map_host(0), gen.height_map_host(0)
    assert np.array_equal(_bits(i0[..., 0]), _bits(rh[..., 0])) and rh[..., 0].any()
    assert np.array_equal(_bits(i0[..., 3]), _bits(rh[..., 3])) and rh[..., 3].any()
    assert np.array_equal(_bits(i1[..., 0]), _bits(rd[..., 0])) and rd[..., 0].any()
    h_err = channel_err(i1[..., 2:3], hm[..., 0:1])[0]
    print(f"N = 2048: image 1 .z against h: {h_err:.2e}, bit for bit: "
          f"{np.array_equal(_bits(i1[..., 2]), _bits(hm[..., 0]))}")
    assert h_err <= 2.0 * FRAME_TOL_GPU, h_err  # each side is held to FRAME_TOL_GPU of the float64 transform
    s = R.settings_dict(gen.GetOceanSettings(0))
    want = K.layer_maps(s, gen.n, gen.initial_spectrum_host(0), depths[1:])[0]
    got = [gen.kinematics_map_host(0, 1, image) for image in range(2)]
    per_image = [channel_err(got[image], want[image]) for image in range(2)]
    errs = [per_image[i][ch] for i, ch in NAMED]
    print("N = 2048, 2-column strips, depth 1 m: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= FRAME_TOL_GPU, errs
    gen.close()
    fft.close()


class _DevicePtr:
    """A device buffer of the library seen by torch (no copy)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


@gpu
def test_layer_zero_is_the_rate_maps_bit_for_bit_8192(ocean):
    """One layer, one cascade at N = 8192: the four-step frame path's 64-column h0 strips; compared on the device."""
    import torch

    from oceansimulation_amd import capi

    n = 8192
    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, 1)
    assert int(capi.lib().ocean_generator_spectrum_block(gen.handle)) == 64
    ocean.apply_settings(gen.GetOceanSettings(0), planeSize=4093.0)
    gen.set_depth_layers((0.0,))
    gen.CalculateOcean(1.0)
    gen.calculate_rates()
    gen.calculate_kinematics()
    fft.synchronize()
    rate = torch.as_tensor(_DevicePtr(capi.lib().ocean_generator_height_rate_map(gen.handle, 0), (2, n, n, 4)), device="cuda")
    kin = torch.as_tensor(_DevicePtr(gen.GetKinematicsMap(0, 0, 0), (2, n, n, 4)), device="cuda")
    for image, ch in ((0, 0), (0, 3), (1, 0)):
        a, b = kin[image, :, :, ch].contiguous().view(torch.int32), rate[image, :, :, ch].contiguous().view(torch.int32)
        assert bool(torch.equal(a, b)), (image, ch)
        assert bool(rate[image, :, :, ch].abs().max() > 0)
    del rate, kin
    torch.cuda.empty_cache()
    gen.close()
    fft.close()


def _scene(ocean, n, depths=DEPTHS, **overrides):
    """Three generators on one plan with their layers: (sampler, host maps, host layer maps, generators)."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(n)
    gens = []
    for plane in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=plane, **overrides)
        g.set_depth_layers(depths)
        g.CalculateOcean(1.0)
        g.calculate_kinematics()
        gens.append(g)
    pairs = [(g, 0) for g in gens]
    layers = [[(g.kinematics_map_host(0, l, 0), g.kinematics_map_host(0, l, 1)) for l in range(len(depths))] for g in gens]
    return SurfaceSampler(pairs), host_cascades(pairs), layers, gens


@pytest.fixture(scope="module")
def calm64(ocean):
    return _scene(ocean, 64)


@gpu
@pytest.mark.parametrize("scene", ["calm", "steep"])
def test_sampler_bit_exact(ocean, oracle, calm64, scene):
    sampler, host, layers, _ = calm64 if scene == "calm" else _scene(ocean, 64, **STEEP)
    xyz, delta = _test_points(lambda xz: sampler.query_host(xz, 8, 0.0)[:, 1])
    got = sampler.kinematics_host(xyz, 8, 0.0)
    want = K.water_kinematics(oracle, host, layers, DEPTHS, xyz, 8, 0.0)
    assert np.array_equal(_bits(got), _bits(want)), np.max(np.abs(got - want))
    _branches_populated(got, delta)
    q = sampler.query_host(xyz[:, [0, 2]].copy(), 8, 0.0)
    assert np.array_equal(_bits(got[:, :4]), _bits(q[:, [0, 1, 2, 7]]))
    speed = np.sqrt((got[:, 4:7].astype(np.float64) ** 2).sum(1))
    print(f"{scene}: mean speed at {BELOW} m under the surface: {[float(speed[delta == np.float32(b)].mean()) for b in BELOW]}")


@gpu
def test_sampler_no_points_and_tolerance(ocean, oracle, calm64):
    """points == 0 launches nothing; a tolerance that stops lanes at different steps still matches."""
    sampler, host, layers, _ = calm64
    assert sampler.kinematics_host(np.zeros((0, 3), np.float32)).shape == (0, 12)
    sampler.kinematics(0, 0, 8, 0.0, 0)  # null pointers with no points
    xyz, _ = _test_points(lambda xz: sampler.query_host(xz, 8, 0.0)[:, 1], count=1000, seed=5)
    got = sampler.kinematics_host(xyz, 3, 1e-3)
    assert np.array_equal(_bits(got), _bits(K.water_kinematics(oracle, host, layers, DEPTHS, xyz, 3, 1e-3)))


@gpu
def test_batched_generator_equals_three_generators(ocean, calm64):
    from oceansimulation_amd.surface import SurfaceSampler

    sampler, _, layers, _ = calm64
    fft = ocean.FFTCalculator(64)
    gen = ocean.Generator(fft, 3)
    for c, plane in enumerate(PLANES):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=plane)
    gen.set_depth_layers(DEPTHS)
    gen.CalculateOcean(1.0)
    gen.calculate_kinematics()
    for c in range(3):
        for l in range(len(DEPTHS)):
            for image in range(2):
                assert np.array_equal(_bits(gen.kinematics_map_host(c, l, image)), _bits(layers[c][l][image])), (c, l, image)
    xyz, _ = _test_points(lambda xz: sampler.query_host(xz, 8, 0.0)[:, 1])
    batched = SurfaceSampler([(gen, c) for c in range(3)])
    assert np.array_equal(_bits(batched.kinematics_host(xyz)), _bits(sampler.kinematics_host(xyz)))
    gen.close()
    fft.close()


@gpu
def test_freshness_and_refusals(ocean):
    from oceansimulation_amd import capi
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.slab import SlabGenerator
    from oceansimulation_amd.surface import SurfaceSampler

    L = capi.lib()
    fft = ocean.FFTCalculator(64)
    gens = [ocean.Generator(fft, 1) for _ in range(2)]
    xyz = np.float32([[1.0, -0.5, 2.0], [30.0, 0.5, -4.0], [3.0, -3.0, 3.0], [0.0, -20.0, 0.0]])
    with pytest.raises(OceanError, match="ocean_generator_calculate_kinematics: no frame"):
        gens[0].calculate_kinematics()
    for g in gens:
        g.CalculateOcean(1.0)
    with pytest.raises(OceanError, match="no depth layers set"):
        gens[0].calculate_kinematics()
    assert gens[0].depth_layers().shape == (0,)
    with pytest.raises(OceanError, match="ascending"):
        gens[0].set_depth_layers((1.0, 0.5))
    for g in gens:
        g.set_depth_layers(DEPTHS)
    assert not L.ocean_generator_kinematics_map(gens[0].handle, 0, 0, 0) and b"never calculated" in L.ocean_last_error()
    with pytest.raises(OceanError):
        gens[0].kinematics_map_host(0, 0, 0)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    gens[0].calculate_kinematics()
    with pytest.raises(OceanError, match="ocean_water_kinematics: generator 1 has no depth layers"):
        sampler.kinematics_host(xyz)
    gens[1].calculate_kinematics()
    assert sampler.kinematics_host(xyz).shape == (4, 12)
    # getter ranges
    base = gens[1].GetKinematicsMap(0, 0, 0)
    assert gens[1].GetKinematicsMap(0, 3, 1) == base + 7 * 64 * 64 * 16
    for c, layer, image in ((1, 0, 0), (0, 4, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        assert not L.ocean_generator_kinematics_map(gens[1].handle, c, layer, image), (c, layer, image)
        assert b"ocean_generator_kinematics_map" in L.ocean_last_error() and b"out of range" in L.ocean_last_error()
    # stale after a frame
    gens[1].CalculateOcean(0.25)
    with pytest.raises(OceanError, match="generator 1 has stale depth layers"):
        sampler.kinematics_host(xyz)
    gens[1].calculate_kinematics()
    assert sampler.kinematics_host(xyz).shape == (4, 12)
    # stale after set_depth_layers, with the same list too
    gens[0].set_depth_layers(DEPTHS)
    with pytest.raises(OceanError, match="generator 0 has stale depth layers"):
        sampler.kinematics_host(xyz)
    gens[0].calculate_kinematics()
    assert sampler.kinematics_host(xyz).shape == (4, 12)
    # another list of the same length on generator 1: named by its index
    gens[1].set_depth_layers((0.0, 0.25, 1.0, 4.5))
    gens[1].calculate_kinematics()
    with pytest.raises(OceanError, match="ocean_water_kinematics: generator 1 has other depth layers"):
        sampler.kinematics_host(xyz)
    # a change of the layer count frees the storage; recalculating works and the getter follows the new count
    for g in gens:
        g.set_depth_layers((0.0, 2.0))
    assert not L.ocean_generator_kinematics_map(gens[0].handle, 0, 0, 0) and b"never calculated" in L.ocean_last_error()
    with pytest.raises(OceanError, match="generator 0 has no depth layers"):
        sampler.kinematics_host(xyz)
    for g in gens:
        g.calculate_kinematics()
    out = sampler.kinematics_host(xyz)
    assert out.shape == (4, 12) and set(out[:, 9]) <= {0.0, 1.0} and out[3, 9] == 1.0
    assert not L.ocean_generator_kinematics_map(gens[0].handle, 0, 2, 0)
    s = R.settings_dict(gens[0].GetOceanSettings(0))
    want = K.layer_maps(s, 64, gens[0].initial_spectrum_host(0), (0.0, 2.0))
    errs = [channel_err(gens[0].kinematics_map_host(0, 1, i), want[1][i])[ch] for i, ch in NAMED]
    assert max(errs) <= FRAME_TOL_GPU, errs
    # argument rules of the query
    with pytest.raises(OceanError, match="ocean_water_kinematics: iterations"):
        sampler.kinematics_host(xyz, 65, 0.0)
    with pytest.raises(OceanError, match="ocean_water_kinematics: tolerance"):
        sampler.kinematics_host(xyz, 8, -1.0)
    slab = SlabGenerator(ocean.FFTCalculator(256), 0, 2)
    assert L.ocean_generator_set_depth_layers(slab.handle, _floats(DEPTHS), 4) == capi.OCEAN_ERR_INVALID
    assert b"slab" in L.ocean_last_error()
    assert L.ocean_generator_calculate_kinematics(slab.handle) == capi.OCEAN_ERR_INVALID and b"slab" in L.ocean_last_error()
    for g in gens:
        g.close()


# ---- the item loops under a CU budget ----------------------------------------------------------------
def _max_resident(wg):
    return min(32, 2048 // wg)


def _bound_holds(wg, items, budget):
    """tests/test_item_loops.py's condition: some workgroup of a budgeted grid runs three or more items."""
    return items >= 3 * budget * _max_resident(wg)


def _fill_sentinel(ptr, nbytes):
    import torch

    from oceansimulation_amd import hip

    s = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hip.copy_d2d(int(ptr), s.data_ptr(), nbytes)
    hip.synchronize()


BUDGETS = (1, 3)
# k_kinematics_pack: 256-thread items. <true> (N >= 64): items = cascades * N^2 / 1024; <false>: cascades * N^2 / 256
PACK_CASES = [dict(id="pack-32x24", n=32, cascades=24, items=24 * 32 * 32 // 256),
              dict(id="pack-128x8", n=128, cascades=8, items=8 * 128 * 128 // 1024)]


@gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=[c["id"] for c in PACK_CASES])
def test_budgeted_layers_equal_full_device(ocean, case):
    """ocean_generator_calculate_kinematics (two layers) under budgets 1 and 3 against the full device, bit for bit,
    on layer maps filled with 0xFF bytes."""
    n, cascades, depths = case["n"], case["cascades"], (0.0, 1.0)
    for b in BUDGETS:
        assert _bound_holds(256, case["items"], b), (case["id"], b)
    nbytes = cascades * len(depths) * 2 * n * n * 16
    gens = []
    for b in (0,) + BUDGETS:
        fft = ocean.FFTCalculator(n)
        gen = ocean.Generator(fft, cascades)
        for c in range(cascades):
            ocean.apply_settings(gen.GetOceanSettings(c), planeSize=17.0, seed=(12342 + 4097 * c, 8934))
        gen.set_depth_layers(depths)
        gen.CalculateOcean(1.0)
        gen.calculate_kinematics()  # allocates the layer maps
        fft.synchronize()
        if b:
            _fill_sentinel(gen.GetKinematicsMap(0, 0, 0), nbytes)
            fft.set_cu_budget(b)
            gen.calculate_kinematics()
            fft.synchronize()
        gens.append((b, fft, gen))
    _, _, full = gens[0]
    want = _bits(ocean.hip.to_host(full.GetKinematicsMap(0, 0, 0), (nbytes // 4,)))
    assert not (want.reshape(-1, 4) == 0xFFFFFFFF).all(axis=1).any()
    for b, _, gen in gens[1:]:
        assert np.array_equal(_bits(ocean.hip.to_host(gen.GetKinematicsMap(0, 0, 0), (nbytes // 4,))), want), (case["id"], b)
    for _, fft, gen in gens:
        gen.close()
        fft.close()


@gpu
def test_budgeted_sampler_equals_full_device(ocean, calm64):
    """ocean_water_kinematics on 24576 points at budgets 1 and 3 against budget 0 on the same plan, bit for bit,
    the output filled with 0xFF bytes first: one thread per point on at most budget * 8 workgroups of 256."""
    from oceansimulation_amd.hip import DeviceBuffer

    sampler, _, _, _ = calm64
    points = 24576
    for b in BUDGETS:
        assert points >= 3 * 8 * 256 * b + 1
    xyz, _ = _test_points(lambda xz: sampler.query_host(xz, 8, 0.0)[:, 1], count=points, seed=17)
    src = DeviceBuffer.from_array(xyz)
    out = DeviceBuffer(points * 48)
    got = {}
    try:
        for b in (0,) + BUDGETS:
            sampler.fft.set_cu_budget(b)
            _fill_sentinel(out.ptr, out.nbytes)
            sampler.kinematics(src.ptr, points, 8, 0.0, out.ptr)
            sampler.fft.synchronize()
            got[b] = out.to_host((points, 12)).view(np.uint32)
    finally:
        sampler.fft.set_cu_budget(0)
    assert not (got[0] == 0xFFFFFFFF).all(axis=1).any()  # no point left unwritten
    for b in BUDGETS:
        assert np.array_equal(got[b], got[0]), b
    src.free()
    out.free()


# ---- the C++ drop-in -------------------------------------------------------------------------------------
CPP_DRIVER = r"""
#include <cstdio>
#include <vector>
#include <hip/hip_runtime.h>
#include "waves/Surface.h"
int main(int argc, char** argv) {
  const float planes[3] = {5.0f, 17.0f, 101.0f};
  const float depths[4] = {0.0f, 0.25f, 1.0f, 4.0f};
  const int points = 512;
  Vision::RenderDevice device;
  Waves::FFTCalculator fft(&device, 64);
  std::vector<Waves::Generator*> gens;
  for (float L : planes) {
    auto* g = new Waves::Generator(&device, &fft);
    g->GetOceanSettings().planeSize = L;
    gens.push_back(g);
  }
  try { gens[0]->CalculateKinematics(); return 2; } catch (const std::exception&) {}  // no frame, no depths
  try { gens[0]->GetKinematicsMap(0, 0); return 2; } catch (const std::exception&) {}
  const float two[2] = {0.0f, 2.0f};
  gens[0]->SetDepthLayers(two, 2);
  for (auto* g : gens) g->CalculateOcean(1.0f, false);
  gens[0]->CalculateKinematics();
  if (device.GetTextureWidth(gens[0]->GetKinematicsMap(1, 1)) != 64) return 3;
  for (auto* g : gens) { g->SetDepthLayers(depths, 4); g->CalculateKinematics(); }  // generator 0: a new layer count
  float back[8];
  if (gens[0]->GetDepthLayers(back) != 4 || back[3] != 4.0f) return 3;
  try { gens[0]->GetKinematicsMap(4, 0); return 2; } catch (const std::exception&) {}
  std::vector<float> xyz(points * 3);
  FILE* in = fopen(argv[1], "rb");
  if (!in || fread(xyz.data(), 4, xyz.size(), in) != xyz.size()) return 4;
  fclose(in);
  float* dev = nullptr;
  if (hipMalloc(&dev, xyz.size() * 4) != hipSuccess) return 4;
  if (hipMemcpy(dev, xyz.data(), xyz.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 4;
  Waves::SurfaceSampler sampler(&device);
  Vision::ID rows = sampler.Kinematics(gens, dev, points, 8, 0.0f);
  device.SubmitCommandBuffer();
  FILE* out = fopen(argv[2], "wb");
  std::vector<float> host(64 * 64 * 4);
  for (auto* g : gens)
    for (int image = 0; image < 2; image++) {
      Vision::ID id = g->GetKinematicsMap(2, image);
      if (hipMemcpy(host.data(), device.GetTexturePointer(id), host.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 5;
      fwrite(host.data(), 4, host.size(), out);
    }
  std::vector<float> got(points * 12);
  if (hipMemcpy(got.data(), device.GetTexturePointer(rows), got.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 5;
  fwrite(got.data(), 4, got.size(), out);
  fclose(out);
  (void)hipFree(dev);
  for (auto* g : gens) delete g;
  return 0;
}
"""


@gpu
def test_cpp_dropin_equals_python(ocean, calm64, tmp_path):
    """Waves::Generator::SetDepthLayers / CalculateKinematics / GetKinematicsMap and SurfaceSampler::Kinematics on the
    scene of the sampler tests: the same bits as the Python layer."""
    sampler, _, layers, _ = calm64
    src, exe = tmp_path / "kinematics_driver.cpp", tmp_path / "kinematics_driver"
    pts, dump = tmp_path / "points.bin", tmp_path / "kinematics.bin"
    src.write_text(CPP_DRIVER)
    xyz, _ = _test_points(lambda xz: sampler.query_host(xz, 8, 0.0)[:, 1], count=512, seed=23)
    pts.write_bytes(xyz.tobytes())
    pkg = os.path.join(ROOT, "oceansimulation_amd")
    r = subprocess.run(["g++", "-O1", "-std=c++17", f"-I{ROOT}/include", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                        "-o", str(exe), str(src), f"-L{pkg}", "-lwaves", "-loceanfft", f"-Wl,-rpath,{pkg}",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(pts), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.frombuffer(dump.read_bytes(), np.uint32)
    per = 64 * 64 * 4
    for c in range(3):
        for image in range(2):
            blob = raw[(2 * c + image) * per:(2 * c + image + 1) * per].reshape(64, 64, 4)
            assert np.array_equal(blob, _bits(layers[c][2][image])), (c, image)
    rows = raw[6 * per:].reshape(512, 12)
    assert np.array_equal(rows, _bits(sampler.kinematics_host(xyz, 8, 0.0)))
