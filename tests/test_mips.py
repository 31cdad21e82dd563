"""Mip pyramids of the maps (ocean_generator_build_mips) and footprint-aware surface sampling
(ocean_surface_sample_lod / _plane_lod), against their contract restated in numpy float32
(tests/surface_lod_ref.py).

The CPU tests pin the restatement itself: on the oracle at footprint 0, on float64 arithmetic for the
level selection and the averaging. The GPU tests compare the kernels with the restatement evaluated on
the GPU's own level-0 maps, bit for bit (np.array_equal): the pyramid's definition fixes the sum order
and the level selection reads the exponent field, so there is no tolerance to choose.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import surface_lod_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
F = np.float32


def _oracle_cascades(oracle, n):
    """The 3-cascade scene of test_surface_query.py on the oracle's maps."""
    out = []
    for L in PLANES:
        g = oracle.OracleGenerator(n, oracle.default_settings(planeSize=L))
        g.calculate_ocean(1.0, True)
        out.append((g.height, g.disp, g.jac, L, g.settings.displacement))
    return out


@pytest.fixture(scope="module")
def oracle64(oracle):
    cas = _oracle_cascades(oracle, 64)
    return cas, R.build_pyramids(cas)


# ---- without a GPU ----------------------------------------------------------------------------
def test_mip_calls_are_exported_and_reject_null_arguments():
    from oceansimulation_amd import capi

    L = capi.lib()
    names = ("ocean_generator_mip_levels", "ocean_generator_build_mips", "ocean_generator_height_mip",
             "ocean_generator_displacement_mip", "ocean_generator_jacobian_mip", "ocean_surface_sample_lod",
             "ocean_surface_sample_plane_lod")
    for name in names:
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    assert L.ocean_generator_mip_levels(None) == 0
    assert L.ocean_generator_build_mips(None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_generator_build_mips" in L.ocean_last_error()
    for name in names[2:5]:
        assert getattr(L, name)(None, 0, 1) is None
        assert name.encode() in L.ocean_last_error()
    assert L.ocean_surface_sample_lod(None, None, 0, None, 0, None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_surface_sample_lod" in L.ocean_last_error()
    cam = (ctypes.c_float * 5)(0.0, 5.0, 0.0, -0.6, 0.8)
    assert L.ocean_surface_sample_plane_lod(None, None, 0, cam, 16, None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_surface_sample_plane_lod" in L.ocean_last_error()
    # 17 pairs: the count rule of ocean_surface_sample, checked before any generator is touched
    gens, cas = (ctypes.c_void_p * 17)(), (ctypes.c_int * 17)()
    assert L.ocean_surface_sample_lod(gens, cas, 17, None, 0, None) == capi.OCEAN_ERR_INVALID
    # a null generator among the pairs
    assert L.ocean_surface_sample_lod(gens, cas, 3, None, 0, None) == capi.OCEAN_ERR_INVALID
    assert b"ocean_surface_sample_lod" in L.ocean_last_error()


def test_reference_at_footprint_zero_is_the_oracle(oracle, oracle64):
    cas, pyr = oracle64
    xz = np.random.default_rng(3).uniform(-150.0, 150.0, (8192, 2)).astype(F)
    xzf = np.concatenate([xz, np.zeros((8192, 1), F)], axis=1)
    got = R.surface_lod(cas, xzf, pyr)
    want = oracle.surface_points(cas, xz)
    assert np.array_equal(got, want), np.max(np.abs(got - want))


def test_lod_of_against_float64():
    top = 12
    rng = np.random.default_rng(0)
    r = np.exp2(rng.uniform(0.0, top, 100000)).astype(F)
    r = r[(r >= 1) & (r < 2.0 ** top)]
    l, f = R.lod_of(r, top)
    want_l = np.floor(np.log2(r.astype(np.float64))).astype(np.int32)
    assert np.array_equal(l, want_l)
    assert np.array_equal(f.astype(np.float64), r.astype(np.float64) / np.exp2(want_l) - 1.0)  # exact in fp32
    assert np.all((f >= 0) & (f < 1))
    # exact at powers of two, f -> 1 just below them
    p2 = np.exp2(np.arange(0, top)).astype(F)
    l, f = R.lod_of(p2, top)
    assert np.array_equal(l, np.arange(0, top)) and np.all(f == 0)
    below = np.nextafter(np.exp2(np.arange(1, top + 1)).astype(F), F(0))
    l, f = R.lod_of(below, top)
    assert np.array_equal(l, np.arange(0, top))
    assert np.all(f == F(1) - F(2.0 ** -23)) and np.all(f < 1)
    # outside the range
    for bad in (0.0, -0.0, -3.0, 0.999, float("nan"), -float("inf")):
        l, f = R.lod_of(np.array([bad], F), top)
        assert (l[0], f[0]) == (0, 0), bad
    for big in (2.0 ** top, 2.0 ** top * 1.5, 1e30, float("inf")):
        l, f = R.lod_of(np.array([big], F), top)
        assert (l[0], f[0]) == (top, 0), big


def test_reference_pyramid_top_is_the_mean(oracle64):
    """Sanity of the fixture, not a kernel tolerance: log2(N) averaging steps in fp32 stay within
    N^2 * 2^-24 of the float64 mean, relative to the largest |texel| of the channel (a channel's mean may
    be arbitrarily close to 0, so the mean itself is no scale; the Jacobian, whose mean is near 1, is
    also held relative to its mean)."""
    cas, pyr = oracle64
    n = 64
    bound = n * n * 2.0 ** -24
    for (h, d, j, _, _), (ph, pd, pj) in zip(cas, pyr):
        for level0, p in ((h, ph), (d, pd), (j.reshape(n, n, 1), pj)):
            assert len(p) == 7 and p[-1].shape[:2] == (1, 1) and all(q.dtype == F for q in p)
            top = p[-1].reshape(-1).astype(np.float64)
            mean = level0.reshape(n * n, -1).astype(np.float64).mean(axis=0)
            scale = np.abs(level0.reshape(n * n, -1)).max(axis=0).astype(np.float64)
            assert np.all(np.abs(top - mean) <= bound * scale), (top, mean)
        jm = j.astype(np.float64).mean()
        assert abs(float(pj[-1].reshape(-1)[0]) - jm) <= bound * abs(jm)


def test_reference_whole_plane_footprint_returns_top_texels(oracle64):
    """A footprint of at least every cascade's planeSize selects (top, 0) everywhere: each sample is its
    cascade's 1 x 1 level times four weights that sum to 1 within 2 ulp, wherever it is taken."""
    cas, pyr = oracle64
    rng = np.random.default_rng(9)
    xz = rng.uniform(-150.0, 150.0, (512, 2))
    for fp in (101.0, 250.0, float("inf")):
        got = R.surface_lod(cas, np.concatenate([xz, np.full((512, 1), fp)], axis=1).astype(F), pyr).astype(np.float64)
        tops_h = [p[0][-1].reshape(4).astype(np.float64) for p in pyr]
        tops_d = [p[1][-1].reshape(4).astype(np.float64) for p in pyr]
        tops_j = [float(p[2][-1].reshape(-1)[0]) for p in pyr]
        scales = [float(F(c[4])) for c in cas]
        x32 = xz.astype(F).astype(np.float64)
        terms_y = [t[0] for t in tops_h]
        terms_x = [s * t[3] for s, t in zip(scales, tops_h)]
        terms_z = [s * t[0] for s, t in zip(scales, tops_d)]
        rtol = 1e-6
        assert np.allclose(got[:, 1], sum(terms_y), rtol=0, atol=rtol * sum(abs(t) for t in terms_y))
        assert np.allclose(got[:, 0], x32[:, 0] + sum(terms_x), rtol=rtol, atol=0)
        assert np.allclose(got[:, 2], x32[:, 1] + sum(terms_z), rtol=rtol, atol=0)
        assert np.allclose(got[:, 3], sum(tops_j) / 3.0, rtol=rtol, atol=0)
        sx = sum(t[1] for t in tops_h) / (1.0 + sum(s * t[1] for s, t in zip(scales, tops_d)))
        sz = sum(t[2] for t in tops_h) / (1.0 + sum(s * t[2] for s, t in zip(scales, tops_d)))
        nrm = np.array([-sx, 1.0, -sz]) / np.sqrt(sx * sx + 1.0 + sz * sz)
        # the slopes are sums of means near 0: absolute against the unit normal
        assert np.allclose(got[:, 4:7], nrm, rtol=0, atol=rtol)


# ---- on the GPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


def _batched(ocean, n, cascades, t=1.0):
    fft = ocean.FFTCalculator(n)
    g = ocean.Generator(fft, cascades)
    for c in range(cascades):
        ocean.apply_settings(g.GetOceanSettings(c), planeSize=PLANES[c % 3])
    g.CalculateOcean(t)
    return fft, g


def _check_pyramid(g, cascades):
    levels = g.mip_levels()
    assert levels == g.n.bit_length()
    for c in range(cascades):
        for level0, getter in ((g.height_map_host(c), g.height_mip_host), (g.displacement_map_host(c), g.displacement_mip_host),
                               (g.jacobian_map_host(c), g.jacobian_mip_host)):
            want = R.pyramid(level0)
            assert len(want) == levels
            for l in range(levels):
                got = getter(c, l)
                assert got.shape == want[l].shape
                assert np.array_equal(got, want[l]), (c, getter.__name__, l, float(np.max(np.abs(got - want[l]))))


@pytest.mark.gpu
@pytest.mark.parametrize("n,cascades", [(16, 1), (32, 1), (64, 1), (128, 1), (256, 3), (4096, 1)])
def test_pyramid_bit_exact(ocean, n, cascades):
    """16, 32: one clipped tile; 64: exactly one tile and one launch; 128: 2 x 2 tiles and a second launch
    on a 2 x 2 source; 256 x 3 cascades: the batch; 4096: two full launches."""
    fft, g = _batched(ocean, n, cascades)
    g.build_mips()
    _check_pyramid(g, cascades)
    g.close()
    fft.close()


@pytest.mark.gpu
def test_pyramid_8192_third_launch(ocean):
    """The third launch (source level 12, a 2 x 2 image): levels >= 4 only are downloaded, each must be the
    box filter of the one below; the first launch's code is held bit for bit at 4096."""
    fft, g = _batched(ocean, 8192, 1)
    g.build_mips()
    assert g.mip_levels() == 14
    for getter in (g.height_mip_host, g.displacement_mip_host, g.jacobian_mip_host):
        below = getter(0, 4)
        assert np.any(below != 0)
        for l in range(4, 13):
            got = getter(0, l + 1)
            assert np.array_equal(got, R.box(below)), (getter.__name__, l + 1)
            below = got
        assert below.shape[:2] == (1, 1)
    g.close()
    fft.close()


@pytest.mark.gpu
def test_rebuild_after_second_frame_and_level_zero(ocean):
    from oceansimulation_amd import capi

    fft, g = _batched(ocean, 128, 2)
    g.build_mips()
    first = g.height_mip_host(1, 3)
    g.CalculateOcean(0.5)
    g.build_mips()
    _check_pyramid(g, 2)  # no level of the first build survives
    assert not np.array_equal(first, g.height_mip_host(1, 3))
    L = capi.lib()
    for c in range(2):
        assert L.ocean_generator_height_mip(g.handle, c, 0) == g.GetHeightMap(c)
        assert L.ocean_generator_displacement_mip(g.handle, c, 0) == g.GetDisplacementMap(c)
        assert L.ocean_generator_jacobian_mip(g.handle, c, 0) == g.GetJacobianMap(c)
    for bad in (-1, 8):
        assert L.ocean_generator_height_mip(g.handle, 0, bad) is None
        assert b"ocean_generator_height_mip" in L.ocean_last_error()
    assert L.ocean_generator_jacobian_mip(g.handle, 2, 1) is None
    g.close()
    fft.close()


@pytest.fixture(scope="module")
def scene256(ocean):
    """WaveApp's 3 x 256^2 scene as three generators with their pyramids built: (sampler, generators,
    host cascades, reference pyramids of the host maps)."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(256)
    gens = []
    for L in PLANES:
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
        g.CalculateOcean(1.0)
        g.build_mips()
        gens.append(g)
    pairs = [(g, 0) for g in gens]
    host = host_cascades(pairs)
    return SurfaceSampler(pairs), gens, host, R.build_pyramids(host)


def _positions():
    rng = np.random.default_rng(7)
    xz = np.concatenate([rng.uniform(-300.0, 300.0, (20000, 2)),
                         np.stack(np.meshgrid(np.arange(-8, 8) * 5.0 / 256.0, [0.0, -5.0, 1e3]), -1).reshape(-1, 2)])
    return xz.astype(F)


@pytest.mark.gpu
def test_sample_lod_bit_exact(ocean, scene256):
    sampler, _, host, pyr = scene256
    xz = _positions()
    pts = xz.shape[0]
    rng = np.random.default_rng(21)
    exact = np.array([2.0 ** j * L / 256.0 for L in PLANES for j in range(0, 9)], F)  # every level boundary
    special = np.array([1e9, np.inf, -1.0], F)
    for name, fp in (("zero", np.zeros(pts, F)),
                     ("level boundaries", exact[np.arange(pts) % exact.size]),
                     ("log-uniform", np.exp(rng.uniform(np.log(1e-3), np.log(1e3), pts)).astype(F)),
                     ("out of range", special[np.arange(pts) % special.size])):
        xzf = np.concatenate([xz, fp[:, None]], axis=1)
        got = sampler.sample_lod_host(xzf)
        want = R.surface_lod(host, xzf, pyr)
        assert np.array_equal(got[:, 7], fp), name
        assert np.array_equal(got, want), (name, float(np.nanmax(np.abs(got - want))))
        assert np.all(np.isfinite(got[:, :7])), name


@pytest.mark.gpu
def test_footprint_zero_is_sample_host(ocean, scene256):
    sampler, _, _, _ = scene256
    xz = _positions()
    got = sampler.sample_lod_host(np.concatenate([xz, np.zeros((xz.shape[0], 1), F)], axis=1))
    assert np.array_equal(got, sampler.sample_host(xz))


@pytest.mark.gpu
def test_plane_lod_bit_exact(ocean, scene256):
    """The plane mesh: the base positions come from the zero-amplitude scene as in
    test_surface_plane_mesh_vs_oracle, the footprints from slot 7; the footprint itself is k * 40 / res
    within 4e-6 relative (that test's 2e-6 for ocml's pow against glibc's, doubled for the one further
    fp32 multiply)."""
    from oceansimulation_amd.surface import SurfaceSampler

    sampler, _, host, pyr = scene256
    cam = [3.0, 5.0, -2.0, -0.6, 0.8]
    res = 128
    flat = []
    for L in PLANES:
        g = ocean.Generator(sampler.fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L, scale=0.0)
        g.CalculateOcean(0.0, update_ocean=True)
        flat.append(g)
    base = SurfaceSampler([(g, 0) for g in flat]).plane_host(cam, res)
    got = sampler.plane_lod_host(cam, res)
    want = R.surface_lod(host, np.concatenate([base[:, [0, 2]], got[:, 7:8]], axis=1), pyr)
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    # the footprint: k recomputed in numpy float32 as the warp computes it
    side = res + 1
    i, j = np.meshgrid(np.arange(side), np.arange(side))
    x = (F(-20.0) + F(40.0) * i.astype(F) / F(res) + F(15.0)).reshape(-1)
    z = (F(-20.0) + F(40.0) * j.astype(F) / F(res) + F(15.0)).reshape(-1)
    fl = np.sqrt(F(cam[3]) * F(cam[3]) + F(cam[4]) * F(cam[4]))
    tx0, tz0 = F(cam[3]) / fl, F(cam[4]) / fl
    tx, tz = (tx0 - tz0) * F(0.70711), (tx0 + tz0) * F(0.70711)
    rx, rz = tx * x - tz * z, x * tz + z * tx
    length = np.sqrt(rx * rx + rz * rz)
    k = np.power(np.maximum(length, F(1.0)), F(1.2)) * F(max(cam[1], 10.0)) * F(0.04)
    fp = k * (F(40.0) / F(res))
    rel = np.abs(got[:, 7].astype(np.float64) - fp) / fp
    print(f"plane footprint: {fp.min():.4f} .. {fp.max():.4f} m, worst relative difference {rel.max():.3e}")
    assert rel.max() <= 4e-6
    for g in flat:
        g.close()


@pytest.mark.gpu
def test_stale_unbuilt_and_slab_are_refused(ocean, scene256):
    from oceansimulation_amd import capi
    from oceansimulation_amd.capi import OceanError
    from oceansimulation_amd.slab import SlabGenerator
    from oceansimulation_amd.surface import SurfaceSampler

    sampler, gens, host, _ = scene256
    xzf = np.array([[1.0, 2.0, 0.5], [-3.0, 4.0, 8.0]], F)
    fresh = ocean.Generator(sampler.fft, 1)
    fresh.CalculateOcean(1.0)
    mixed = SurfaceSampler([(gens[0], 0), (fresh, 0)])
    for call in (lambda: mixed.sample_lod_host(xzf), lambda: mixed.plane_lod_host([3.0, 5.0, -2.0, -0.6, 0.8], 8)):
        with pytest.raises(OceanError) as e:  # never built
            call()
        assert e.value.code == capi.OCEAN_ERR_INVALID and "generator 1" in str(e.value)
    fresh.build_mips()
    mixed.sample_lod_host(xzf)
    fresh.CalculateOcean(0.1)  # the maps are rewritten: the pyramid is stale
    with pytest.raises(OceanError) as e:
        mixed.sample_lod_host(xzf)
    assert e.value.code == capi.OCEAN_ERR_INVALID and "generator 1" in str(e.value)
    fresh.build_mips()
    mixed.sample_lod_host(xzf)
    mixed.sample_host(xzf[:, :2].copy())  # the level-0 calls never needed a pyramid
    slab = SlabGenerator(ocean.FFTCalculator(256), 0, 2)
    assert capi.lib().ocean_generator_build_mips(slab.handle) == capi.OCEAN_ERR_INVALID
    assert b"ocean_generator_build_mips" in capi.lib().ocean_last_error()
    fresh.close()


@pytest.mark.gpu
def test_batched_generator_cascade_one(ocean):
    """(generator, cascade) pairs into one batched generator: cascade 1's chain, not cascade 0's."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft, g = _batched(ocean, 64, 3)
    g.build_mips()
    pairs = [(g, 1), (g, 2)]
    host = host_cascades(pairs)
    rng = np.random.default_rng(4)
    xzf = np.concatenate([rng.uniform(-60.0, 60.0, (4097, 2)), np.exp(rng.uniform(np.log(1e-2), np.log(2e2), (4097, 1)))],
                         axis=1).astype(F)
    got = SurfaceSampler(pairs).sample_lod_host(xzf)
    assert np.array_equal(got, R.surface_lod(host, xzf))
    g.close()
    fft.close()


@pytest.mark.gpu
def test_waveapp_headless_mips(ocean, tmp_path):
    exe = os.path.join(ROOT, "examples", "waveapp_headless")
    r = subprocess.run([exe, "--n", "64", "--frames", "3", "--mesh", "32", "--mips", "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mips"] == 7
    for i in range(3):
        want = R.pyramid(np.load(tmp_path / f"height_{i}.npy"))
        assert np.array_equal(np.load(tmp_path / f"height_{i}_mip1.npy"), want[1])
        assert np.array_equal(np.load(tmp_path / f"height_{i}_mip6.npy"), want[6])
    mesh = np.load(tmp_path / "mesh_lod.npy")
    assert mesh.shape == (33 * 33, 8) and np.all(np.isfinite(mesh))
    assert np.all(mesh[:, 7] > 0)
    # without the switch nothing changes
    r = subprocess.run([exe, "--n", "64", "--frames", "1", "--mesh", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mips" not in json.loads(r.stdout.strip().splitlines()[-1])
