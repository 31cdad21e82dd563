"""Standalone EncodeIFFT at the shapes the other tests do not reach: the 16-column k_cols<8..10> (batches of
>= 256 strips, or one image under a small CU budget), item loops of k_rows_ifft / k_cols / k_cols_to_blocks /
k_cols_pre / k_rows_final under budgets, and the in-place passes that serve 4096 / 8192 when the work image
cannot be allocated (k_cols<12>, k_cols<13>, k_cols<14>; ocean_debug_fft_work_limit), and the 16384 four-step
path under a budget.

Inputs are test_gpu_parity._rand_image, the reference numpy_ref.encode_ifft in float64, the gate FFT_TOL per
lane and per image (tests/parity.py). launch_cols (launch_fft.hip) picks the narrow k_cols<LOGN, 2, 4> only at
256 <= N <= 1024 when items < cus, items = images * N / 16 and cus the plan's budget (the device's CUs without
one), and the 16-column k_cols<LOGN> otherwise; two runs that select the same kernel must agree bit for bit,
whatever their grids. Observed float64 errors: profiles/item_loops.md.
"""
import numpy as np
import pytest

import numpy_ref as R
from parity import FFT_TOL, lane_err
from test_gpu_parity import _rand_image
from test_item_loops import bound_holds

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


# ---- launch_fft.hip, restated ------------------------------------------------------------------------
def col_cfg(n):
    """device/grid.h ColCfg: columns per strip, workgroup size, strips per image."""
    t = n // 16
    c = 1 if t >= 1024 else min(16, 1024 // t)
    return dict(C=c, WG=t * c, STRIPS=n // c)


def row_cfg(n):
    """device/k_fft.h RowCfg: rows per item, workgroup size."""
    t = n // 16
    rpw = 1 if t >= 256 else 256 // t
    return dict(RPW=rpw, WG=t * rpw)


def selects_wide(n, images, cus):
    """launch_cols: the narrow kernel exists at 256 <= N <= 1024 (C > 4, LOGN >= 8) and is taken when items < cus."""
    k = col_cfg(n)
    return not (k["C"] > 4 and n >= 256 and images * k["STRIPS"] < cus)


def _ifft(fft, imgs):
    from oceansimulation_amd.hip import DeviceBuffer

    buf = DeviceBuffer.from_array(imgs)
    fft.encode_ifft_batch(buf.ptr, imgs.shape[0])
    fft.synchronize()
    out = buf.to_host(imgs.shape)
    buf.free()
    return out


def _kat_image(n):
    """test_kat_delta_and_plane_wave's input: a delta at the centred DC on lane 0, one bin on lane 1."""
    img = np.zeros((n, n, 4), np.float32)
    img[n // 2, n // 2, 0] = 1.0
    kx, ky = 3, n // 2 - 5
    img[n // 2 + ky, n // 2 + kx, 2] = 1.0
    return img, kx, ky


def _check_kat(got, n, kx, ky):
    assert np.allclose(got[..., 0], 1.0, atol=1e-6) and np.allclose(got[..., 1], 0.0, atol=1e-6)
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    ph = 2 * np.pi * ((kx * x + ky * y) % n) / n
    assert np.max(np.abs(got[..., 2] - np.cos(ph))) < 2e-5
    assert np.max(np.abs(got[..., 3] - np.sin(ph))) < 2e-5


# ---- wide k_cols on the full device -------------------------------------------------------------------
# (N, images): images * N / 16 strips >= 256 CUs select k_cols<8>, <9>, <10> with 16 columns per strip. The
# second three end on an odd image count, so the last image starts at a strip that is no multiple of 256.
# N / 16 is a multiple of 16 at every one of these sizes, so a one-shot grid is always a multiple of 16 and the
# slot map of these runs is the permuted one; the identity branch is reached by the budgets 1 and 3 below.
WIDE_BATCHES = [(256, 16), (512, 8), (1024, 4), (256, 17), (512, 9), (1024, 5)]


@gpu
@pytest.mark.parametrize("n,images", WIDE_BATCHES)
def test_wide_cols_batches_vs_float64(ocean, n, images):
    fft = ocean.FFTCalculator(n)
    items = images * col_cfg(n)["STRIPS"]
    assert items >= fft.cus and selects_wide(n, images, fft.cus), (items, fft.cus)
    kat, kx, ky = _kat_image(n)
    imgs = np.stack([_rand_image(n, 1000 * n + i) for i in range(images - 1)] + [kat])
    got = _ifft(fft, imgs)
    worst = 0.0
    for i in range(images):
        errs = lane_err(got[i], R.encode_ifft(imgs[i]))
        worst = max(worst, max(errs))
        assert max(errs) <= FFT_TOL, (n, images, i, errs)
    _check_kat(got[-1], n, kx, ky)
    print(f"wide k_cols N = {n}, {images} images: worst lane error {worst:.2e}")
    fft.close()


# ---- one image (two at 1024 / budget 64) under budgets -------------------------------------------------
# (N, images, budget). k_rows_ifft: 256-thread items of RPW rows; k_cols<LOGN>: WG = T * C. `loops` names the
# kernels whose three-items bound holds for the row (asserted); the other rows are there for the float64
# comparison and the kernel choice.
BUDGET_RUNS = [
    (16, 1, 1, ()), (16, 1, 3, ()), (16, 1, 16, ()),
    (64, 1, 1, ()), (64, 1, 3, ()), (64, 1, 16, ()),
    (256, 1, 1, ()), (256, 1, 3, ()), (256, 1, 16, ()),
    (256, 2, 1, ("k_rows_ifft", "k_cols")),                      # 32 row items, 32 strips >= 24
    (512, 1, 1, ("k_rows_ifft", "k_cols")), (512, 1, 3, ()), (512, 1, 16, ()),
    (1024, 1, 1, ("k_rows_ifft", "k_cols")), (1024, 1, 3, ("k_rows_ifft", "k_cols")), (1024, 1, 16, ()),
    (1024, 2, 64, ()),                                            # 128 items >= 64: wide
    (2048, 1, 1, ("k_rows_ifft", "k_cols")), (2048, 1, 3, ("k_rows_ifft", "k_cols")),
    (2048, 1, 16, ("k_rows_ifft", "k_cols")),
]


@pytest.fixture(scope="module")
def budget_refs():
    """float64 transforms of the images of BUDGET_RUNS, computed once per (N, image)."""
    cache = {}

    def get(n, i):
        if (n, i) not in cache:
            img = _rand_image(n, 7 * n + i)
            cache[(n, i)] = (img, R.encode_ifft(img))
        return cache[(n, i)]

    return get


@gpu
@pytest.mark.parametrize("n", sorted({r[0] for r in BUDGET_RUNS}))
def test_budgeted_ifft_vs_float64_and_each_other(ocean, budget_refs, n):
    """Every run of the size against float64; image 0 of every run that selects the wide kernel is bit for bit
    the same (the row pass has one kernel per size), and equals the full device's when that selects it too."""
    wide_bits = None
    for rn, images, budget, loops in BUDGET_RUNS:
        if rn != n:
            continue
        rows, cols = row_cfg(n), col_cfg(n)
        assert selects_wide(n, images, budget), (n, images, budget)
        if "k_rows_ifft" in loops:
            assert bound_holds(rows["WG"], -(-images * n // rows["RPW"]), budget), (n, images, budget)
        if "k_cols" in loops:
            assert bound_holds(cols["WG"], images * cols["STRIPS"], budget), (n, images, budget)
        fft = ocean.FFTCalculator(n)
        fft.set_cu_budget(budget)
        imgs = np.stack([budget_refs(n, i)[0] for i in range(images)])
        got = _ifft(fft, imgs)
        for i in range(images):
            errs = lane_err(got[i], budget_refs(n, i)[1])
            print(f"N = {n}, {images} image(s), budget {budget}, image {i}: lane errors {errs[0]:.2e} {errs[1]:.2e}")
            assert max(errs) <= FFT_TOL, (n, images, budget, i, errs)
        if wide_bits is None:
            wide_bits = got[0]
        assert np.array_equal(got[0], wide_bits), (n, images, budget)
        fft.close()
    fft = ocean.FFTCalculator(n)
    if selects_wide(n, 1, fft.cus):
        assert np.array_equal(_ifft(fft, budget_refs(n, 0)[0][None])[0], wide_bits), n
    fft.close()


# ---- column-first (4096) and pre-stage (8192) under budgets -------------------------------------------
# k_cols_to_blocks<12>: 1024 threads, images * 1024 strips; k_rows_final<12, ..., RPW 1>: 256 threads, images * 4096
# k_cols_pre<13>: 1024 threads, images * 2048 * 2 items; k_rows_final<13, ..., RPW 1>: 512 threads, images * 8192
WORK_IMAGE_RUNS = [
    dict(n=4096, images=3, kernels=[("k_cols_to_blocks", 1024, 3 * 1024), ("k_rows_final", 256, 3 * 4096)]),
    dict(n=8192, images=2, kernels=[("k_cols_pre", 1024, 2 * 2048 * 2), ("k_rows_final", 512, 2 * 8192)]),
]


@gpu
@pytest.mark.parametrize("run", WORK_IMAGE_RUNS, ids=[str(r["n"]) for r in WORK_IMAGE_RUNS])
def test_work_image_paths_budgets_equal_full_device(ocean, run):
    """Budgets 1 and 16 against the full device, bit for bit, compared on the device (the full-device side is
    pinned to float64 by test_encode_ifft_large_vs_float64)."""
    import torch

    n, images = run["n"], run["images"]
    for name, wg, items in run["kernels"]:
        for b in (1, 16):
            assert bound_holds(wg, items, b), (name, b)
    src = torch.randn((images, n, n, 4), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    outs = []
    for budget in (0, 1, 16):
        fft = ocean.FFTCalculator(n)
        fft.set_cu_budget(budget)
        buf = src.clone()
        torch.cuda.synchronize()
        fft.encode_ifft_batch(buf.data_ptr(), images)
        fft.synchronize()
        outs.append(buf)
        fft.close()
    assert not torch.equal(outs[0], src) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]), (n, "budget 1")
    assert torch.equal(outs[0], outs[2]), (n, "budget 16")


# ---- the in-place fallback at 4096 / 8192 / 16384, four-step 16384 under a budget ---------------------------------------------------------------
@gpu
def test_in_place_fallback_4096(ocean):
    """Work limit 0 at 4096: launch_rows_ifft + launch_cols with k_cols<12> (4 columns per strip, 1024 strips)
    against float64; two images at budget 3 (k_rows_ifft: 8192 items, k_cols<12>: 2048) equal the one-image
    results bit for bit; with the limit lifted the plan is column-first again, bit for bit a fresh plan's."""
    n = 4096
    a, b = _rand_image(n, 99), _rand_image(n, 98)
    fresh = ocean.FFTCalculator(n)
    colfirst = _ifft(fresh, a[None])[0]
    fresh.close()
    fft = ocean.FFTCalculator(n)
    assert np.array_equal(_ifft(fft, a[None])[0], colfirst)  # holds a work image now
    fft.debug_work_limit(0)  # frees it
    in_place_a = _ifft(fft, a[None])[0]
    errs = lane_err(in_place_a, R.encode_ifft(a))
    print(f"in-place 4096: lane errors {errs[0]:.2e} {errs[1]:.2e}")
    assert max(errs) <= FFT_TOL, errs
    assert not np.array_equal(in_place_a, colfirst)  # another order of the passes: other roundings
    in_place_b = _ifft(fft, b[None])[0]
    assert bound_holds(row_cfg(n)["WG"], 2 * n, 3) and bound_holds(col_cfg(n)["WG"], 2 * col_cfg(n)["STRIPS"], 3)
    fft.set_cu_budget(3)
    both = _ifft(fft, np.stack([a, b]))
    assert np.array_equal(both[0], in_place_a) and np.array_equal(both[1], in_place_b)
    fft.set_cu_budget(0)
    fft.debug_work_limit(None)
    assert np.array_equal(_ifft(fft, a[None])[0], colfirst)
    fft.close()


# (N, budget, work limit): the separable input of test_encode_ifft_separable_vs_float64, whose float64 reference
# costs two 1D transforms, so each case costs what that test costs at its size.
#   8192, limit 0: k_rows_ifft<13> + k_cols<13> (2 columns per strip) in place.
#   16384, budget 100: the four-step path on persistent grids: k_rows_ifft<14> (16384 items of 1024 threads),
#     k_cols4_step1 (8192 items of 256 per 2048-column slab), k_cols4_step2<10> (2048 items of 1024).
#   16384, limit 0: k_rows_ifft<14> + k_cols<14> (one column per strip) in place.
SEPARABLE_RUNS = [
    dict(id="8192-in-place", n=8192, budget=0, limit=0, kernels=[]),
    dict(id="16384-four-step-budget-100", n=16384, budget=100, limit=None,
         kernels=[("k_rows_ifft", 1024, 16384), ("k_cols4_step1", 256, (2048 // 64) * (1024 // 4)),
                  ("k_cols4_step2", 1024, 16 * (2048 // 16))]),
    dict(id="16384-in-place", n=16384, budget=0, limit=0, kernels=[]),
]


@gpu
@pytest.mark.parametrize("run", SEPARABLE_RUNS, ids=[r["id"] for r in SEPARABLE_RUNS])
def test_separable_vs_float64(ocean, run):
    """256 random rows of the transform of a sum of two outer products per lane against float64 at FFT_TOL."""
    from oceansimulation_amd.hip import DeviceBuffer

    n = run["n"]
    for name, wg, items in run["kernels"]:
        assert bound_holds(wg, items, run["budget"]), (name, wg, items)
    rng = np.random.default_rng(n)
    a = rng.standard_normal((2, 2, n)) + 1j * rng.standard_normal((2, 2, n))  # [term, lane, y]
    b = rng.standard_normal((2, 2, n)) + 1j * rng.standard_normal((2, 2, n))  # [term, lane, x]
    img = np.empty((n, n, 4), np.float32)
    for lane in range(2):
        m = np.einsum("ty,tx->yx", a[:, lane].astype(np.complex64), b[:, lane].astype(np.complex64))
        img[..., 2 * lane], img[..., 2 * lane + 1] = m.real, m.imag
        del m
    a64, b64 = a.astype(np.complex64).astype(np.complex128), b.astype(np.complex64).astype(np.complex128)
    fa = n * np.fft.ifft(np.fft.ifftshift(a64, axes=-1), axis=-1)
    fb = n * np.fft.ifft(np.fft.ifftshift(b64, axes=-1), axis=-1)
    fft = ocean.FFTCalculator(n)
    fft.set_cu_budget(run["budget"])
    if run["limit"] is not None:
        fft.debug_work_limit(run["limit"])
    buf = DeviceBuffer.from_array(img)
    del img
    fft.EncodeIFFT(buf.ptr)
    fft.synchronize()
    got = buf.to_host((n, n, 4))
    buf.free()
    rows = np.sort(rng.choice(n, 256, replace=False))
    for lane in range(2):
        ref = np.einsum("ty,tx->yx", fa[:, lane, rows], fb[:, lane])
        g = got[rows][..., 2 * lane] + 1j * got[rows][..., 2 * lane + 1]
        err = np.abs(g - ref).max() / np.abs(ref).max()
        print(f"{run['id']}, lane {lane}: {err:.2e}")
        assert err <= FFT_TOL, (run["id"], lane, err)
    fft.close()


def test_kernel_choice_restated():
    """The `items < cus` rule on a 256-CU device: one image takes the narrow kernel at 256 .. 1024 and the wide
    one under every budget of BUDGET_RUNS; 2048 and the sizes below 256 have one column kernel."""
    for n in (256, 512, 1024):
        assert not selects_wide(n, 1, 256)
        assert all(selects_wide(n, 1, b) for b in (1, 3, 16))
    assert selects_wide(1024, 2, 64) and not selects_wide(1024, 1, 65)
    assert all(selects_wide(n, 1, 256) for n in (16, 64, 2048, 4096, 8192))
    assert [col_cfg(n)["STRIPS"] for n in (256, 512, 1024, 2048, 4096, 8192)] == [16, 32, 64, 256, 1024, 4096]
