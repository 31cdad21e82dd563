"""Every kernel's item loop past its first item: frames, rates, slabs, hull loads and surface requests under a CU budget.

Every frame kernel is a loop `for (item = slot(blockIdx.x, gridDim.x); item < total; item += gridDim.x)`
whose body reuses the LDS exchange, the twiddle table and (some) loads carried from one item to the next.
On a plan that owns the device persistent_grid() (launch_common.h) gives one workgroup per item, so the
loop body runs once. Under ocean_fft_set_cu_budget the grid is blocks_per_cu x budget and the loops run.

The condition that makes a case count, asserted from the tables below and not measured: a workgroup of WG
threads is resident at most min(32, 2048 / WG) times per CU (32 workgroup slots, 2048 threads), so a
budgeted grid has at most budget * min(32, 2048 / WG) workgroups, and with
    items >= 3 * budget * min(32, 2048 / WG)
some workgroup runs three or more items. WG and items are restated here from the launchers (ColFirstCfg,
FftShape, ColsLaunch::items, launch_*); each row names the kernels it is there for and the budgets at
which the bound holds for them. Budgets 1 and 3 give grids that are no multiple of 16 (the identity
branch of xcd_group_slot / xcd_pair_slot, for every resident count that is no multiple of 16 itself);
budgets 16 and 32 give per_cu * 16 / per_cu * 32 workgroups, a multiple of 8 * GROUP for every GROUP in
use (the permuted branch).

Budgeted and full-device generators live at the same time on plans of their own; the budgeted maps are
filled with 0xFF bytes before the first frame, so an item that is skipped cannot pass on recycled memory.
"""
import numpy as np
import pytest

import numpy_ref as R
import settings_cases
from parity import FRAME_TOL_GPU
from test_gpu_parity import _frame_check

gpu = pytest.mark.gpu

PLANE = 17.0


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


# ---- the launchers' geometry, restated ---------------------------------------------------------------
def max_resident(wg):
    return min(32, 2048 // wg)


def bound_holds(wg, items, budget):
    return items >= 3 * budget * max_resident(wg)


def col_first_cfg(n):
    """device/grid.h ColFirstCfg: B, SPW, WG1 (k_cols_evolve), RPW2, WG2 (k_rows_final)."""
    t = n // 16
    b = 1 if t >= 1024 else 2 if t >= 512 else min(t, 4)
    spw = max(1, (256 if t >= 64 else 64) // (t * b))
    spw = min(spw, n // b)
    rpw2 = 64 // t if t < 64 else (256 // t if 256 // t >= 4 else min(1024 // t, 4))
    rpw2 = min(rpw2, n)
    return dict(T=t, B=b, SPW=spw, WG1=t * b * spw, RPW2=rpw2, WG2=t * rpw2)


def full_kernels(n, c):
    """launch_cols_evolve / launch_rows_final (launch_fft.hip): (name, WG, items)."""
    k = col_first_cfg(n)
    return [("k_cols_evolve", k["WG1"], c * ((n // k["B"]) // k["SPW"])),
            ("k_rows_final", k["WG2"], c * 2 * (n // k["RPW2"]))]


def half_kernels(n, c):
    """launch_half_columns / launch_half_rows (launch_half.hip): half strips (CPI 2, FB 2 fields) at 2048 /
    4096 with <= 2 cascades, whole strips otherwise; rows: k_rows_hp at 4096, k_rows_half below. The column
    grid is also capped by the H scratch slices (max_grid = device CUs * 1024 / WG): on the full device
    k_cols_half already loops whenever items exceed that, which the full-device side of every case runs."""
    t, strips = n // 16, n // 8 + 1
    half_strip = n in (2048, 4096) and c <= 2
    cpi = 2 if half_strip else 4
    cols = ("k_cols_half<ColsHalfStrip>" if half_strip else "k_cols_half<ColsWhole>", t * cpi, c * strips * (4 // cpi))
    if n == 4096:
        rows = ("k_rows_hp<FB 2>" if half_strip else "k_rows_hp<FB 4, EARLY 1, MINB 3>", 256, c * n)
    else:
        rows = ("k_rows_half<RowsHalf<%d>>" % (2 if half_strip else 4), t * 2, c * (n // 2))
    return [cols, rows]


def gen4_kernels(n, c):
    """launch_gen4_columns / launch_gen4_rows (launch_slab.hip) of a whole grid (one rank), N = 8192."""
    assert n == 8192
    ncols = n // 2 + 1
    return [("k_gen4_step1", 256, c * ((ncols + 63) // 64) * ((n // 16) // 4)),
            ("k_gen4_step2", 512, c * 16 * ((ncols + 15) // 16)),              # N2 = 512: T 32 x CI 16
            ("k_gen4_step2 (gc)", 512, c * 16 * (((ncols + 1) // 2 + 15) // 16)),
            ("k_rows_half<row-major>", (n // 16) * 2, c * (n // 2))]             # launch_rm_rows, RPW 2


def half_to_rows_tiles(n, c, ranks):
    """launch_half_slab_rows: tiles of k_half_to_rows (256 u x 16 y), per cascade and source block."""
    b = col_first_cfg(n)["B"]
    strips = n // (2 * b) + 1
    s = -(-strips // ranks)
    return c * (-(-strips // s)) * (-(-(s * b) // 256)) * ((n // ranks) // 16)


def strip_dealt_kernels(n, c):
    """The strip-dealt column pass of a whole grid (ColsSlab, one workgroup per scratch slice), the move to
    row-major fields (k_half_to_rows: its own grid of cus * 4) and launch_rm_rows, N = 8192."""
    k = col_first_cfg(n)
    return [("k_cols_half<ColsSlab>", k["T"] * k["B"], c * (n // (2 * k["B"]) + 1)),
            ("k_rows_half<row-major>", k["T"] * 2, c * (n // 2))]


def _kernels(case):
    return {"full": full_kernels, "half": half_kernels, "gen4": gen4_kernels,
            "strips": strip_dealt_kernels}[case["path"]](case["n"], case["cascades"])


# ---- the frame cases ---------------------------------------------------------------------------------
# path: full = full spectrum, half = blocked half spectrum, gen4 = four-step (8192), strips = strip-dealt (8192)
# budgets: the budgets the case runs at; counts: {kernel name: budgets at which the bound must hold}
# oracle: the budgeted maps are also checked with _frame_check (smallest N of each formulation)
FRAME_CASES = [
    # k_cols_evolve<6> (64-thread items, 4 per cascade), k_rows_final<6> (8 per cascade): budget 1 only
    dict(id="full-64x32", n=64, cascades=32, path="full", budgets=(1,), oracle=True,
         counts={"k_cols_evolve": (1,), "k_rows_final": (1,)}),
    # k_cols_evolve<8>, k_rows_final<8>; budget 3 (identity branch) counts for the row pass
    dict(id="full-256x3", n=256, cascades=3, path="full", budgets=(1, 3), oracle=True,
         counts={"k_cols_evolve": (1,), "k_rows_final": (1, 3)}),
    # k_cols_evolve<9>, k_rows_final<9>, finite depth and the spectral peak (peak_shallow)
    dict(id="full-512x2-peak_shallow", n=512, cascades=2, path="full", budgets=(1, 3), settings="peak_shallow",
         counts={"k_cols_evolve": (1, 3), "k_rows_final": (1, 3)}),
    # k_cols_evolve<10>, k_rows_final<10> (256-thread items); budget 16: the row pass
    dict(id="full-1024x1", n=1024, cascades=1, path="full", budgets=(3, 16),
         counts={"k_cols_evolve": (3,), "k_rows_final": (3, 16)}),
    # the same with two cascades, so that budget 16 counts for k_cols_evolve<10> too
    dict(id="full-1024x2", n=1024, cascades=2, path="full", budgets=(16,),
         counts={"k_cols_evolve": (16,), "k_rows_final": (16,)}),
    # ColsWhole<10>, RowsHalf<4>
    dict(id="half-1024x1", n=1024, cascades=1, path="half", budgets=(1, 3), oracle=True,
         counts={"k_cols_half<ColsWhole>": (1, 3), "k_rows_half<RowsHalf<4>>": (1, 3)}),
    dict(id="half-1024x3", n=1024, cascades=3, path="half", budgets=(3, 16),
         counts={"k_cols_half<ColsWhole>": (3, 16), "k_rows_half<RowsHalf<4>>": (3, 16)}),
    # frame overlap: the second field set and the internal stream under a budget
    dict(id="half-1024x1-overlap", n=1024, cascades=1, path="half", budgets=(3,), overlap=True,
         counts={"k_cols_half<ColsWhole>": (3,), "k_rows_half<RowsHalf<4>>": (3,)}),
    # half strips (ColsHalfStrip<11>), RowsHalf<2>
    dict(id="half-2048x1", n=2048, cascades=1, path="half", budgets=(1, 16),
         counts={"k_cols_half<ColsHalfStrip>": (1, 16), "k_rows_half<RowsHalf<2>>": (1, 16)}),
    # ColsWhole<11>
    dict(id="half-2048x3", n=2048, cascades=3, path="half", budgets=(3, 32),
         counts={"k_cols_half<ColsWhole>": (3, 32), "k_rows_half<RowsHalf<4>>": (3, 32)}),
    # half strips (ColsHalfStrip<12>), RowsHp<2, ...>
    dict(id="half-4096x1", n=4096, cascades=1, path="half", budgets=(3, 32),
         counts={"k_cols_half<ColsHalfStrip>": (3, 32), "k_rows_hp<FB 2>": (3, 32)}),
    # ColsWhole<12>, RowsHp<4, ..., EARLY 1, MINB 3>: image 1's loads before image 0's stores
    dict(id="half-4096x3", n=4096, cascades=3, path="half", budgets=(1, 32),
         counts={"k_cols_half<ColsWhole>": (1, 32), "k_rows_hp<FB 4, EARLY 1, MINB 3>": (1, 32)}),
    # k_gen4_step1 / k_gen4_step2, k_rows_half on the row-major fields of the exchange blocks
    dict(id="gen4-8192", n=8192, cascades=1, path="gen4", budgets=(32,),
         counts={"k_gen4_step1": (32,), "k_gen4_step2": (32,), "k_gen4_step2 (gc)": (32,),
                 "k_rows_half<row-major>": (32,)}),
    # strip-dealt column pass (ColsSlab<13>), k_half_to_rows on its cus * 4 grid, k_rows_half row-major
    dict(id="strips-8192", n=8192, cascades=1, path="strips", budgets=(32,), half_to_rows=True,
         counts={"k_cols_half<ColsSlab>": (32,), "k_rows_half<row-major>": (32,)}),
]


def test_case_table_meets_the_three_items_bound():
    """Every (kernel, budget) a case claims satisfies items >= 3 * budget * min(32, 2048 / WG); every case
    claims at least one; between them the cases reach a small budget (identity slot map) and a budget that is
    a multiple of 16 (permuted slot map) for the column and the row kernels of every formulation."""
    for case in FRAME_CASES:
        kernels = {name: (wg, items) for name, wg, items in _kernels(case)}
        assert set(case["counts"]) <= set(kernels), (case["id"], sorted(kernels))
        assert any(case["counts"].values()), case["id"]
        for name, budgets in case["counts"].items():
            wg, items = kernels[name]
            for b in budgets:
                assert b in case["budgets"], (case["id"], name, b)
                assert bound_holds(wg, items, b), (case["id"], name, wg, items, b)
        if case.get("half_to_rows"):  # its grid is exactly budget * 4 workgroups once tiles >= that
            for b in case["budgets"]:
                assert half_to_rows_tiles(case["n"], case["cascades"], 1) >= 3 * b * 4, case["id"]
    reached = {}
    for case in FRAME_CASES:
        for name, budgets in case["counts"].items():
            reached.setdefault(name.split("<")[0], set()).update(budgets)
    for name in ("k_cols_evolve", "k_rows_final", "k_cols_half", "k_rows_half", "k_rows_hp"):
        assert reached[name] & {1, 3} and reached[name] & {16, 32}, (name, reached[name])
    assert reached["k_gen4_step1"] == {32} and reached["k_gen4_step2"] == {32}


# ---- device buffers ----------------------------------------------------------------------------------
def _fill_sentinel(ptr, nbytes):
    import torch

    from oceansimulation_amd import hip

    s = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hip.copy_d2d(int(ptr), s.data_ptr(), nbytes)
    hip.synchronize()


def _dev_copy(ptr, nbytes):
    import torch

    from oceansimulation_amd import hip

    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip.copy_d2d(t.data_ptr(), int(ptr), nbytes)
    return t


def _same_on_device(a_ptr, b_ptr, nbytes):
    import torch

    return bool(torch.equal(_dev_copy(a_ptr, nbytes), _dev_copy(b_ptr, nbytes)))


def _map_ptrs(gen, c):
    n = gen.n
    return (("height", gen.GetHeightMap(c), n * n * 16), ("displacement", gen.GetDisplacementMap(c), n * n * 16),
            ("jacobian", gen.GetJacobianMap(c), n * n * 4))


def _case_settings(case, c):
    if case.get("settings"):
        s = dict(settings_cases.settings(case["settings"], case["n"]))
    else:
        s = dict(planeSize=PLANE)
    s["seed"] = (12342 + 4097 * c, 8934)  # same plane for every cascade: the seed tells them apart
    return s


def _make_generator(ocean, case, budget):
    fft = ocean.FFTCalculator(case["n"])
    fft.set_cu_budget(budget)
    gen = ocean.Generator(fft, case["cascades"])
    if case["path"] == "full" and case["n"] >= 1024:
        gen.set_half_spectrum(False)
    if case["path"] == "strips":
        gen.set_four_step(False)
    gen.set_h0_memo(False)
    if case.get("overlap"):
        gen.set_frame_overlap(True)
    for c in range(case["cascades"]):
        ocean.apply_settings(gen.GetOceanSettings(c), **_case_settings(case, c))
    return fft, gen


FRAMES = ((0.25, False), (1.0 / 60.0, False), (1.0 / 60.0, True))  # the third: after a settings edit, memo off


@gpu
@pytest.mark.parametrize("case", FRAME_CASES, ids=[c["id"] for c in FRAME_CASES])
def test_budgeted_frames_equal_full_device(ocean, oracle, case):
    """Three frames (dt 0.25, 1/60, then a re-seed after a settings edit with the h0 memo off: the seeding
    column-pass variants) under each budget of the case against the full device, bit for bit after every
    frame: height, displacement, Jacobian, and h0 after the first and third frame. The smallest N of each
    formulation also checks the budgeted maps against the oracle and its float64 transform (_frame_check)."""
    n, cascades = case["n"], case["cascades"]
    full_fft, full = _make_generator(ocean, case, 0)
    budgeted = [(b,) + _make_generator(ocean, case, b) for b in case["budgets"]]
    for _, _, gen in budgeted:
        for c in range(cascades):
            for _, ptr, nb in _map_ptrs(gen, c):
                _fill_sentinel(ptr, nb)
    refs = []
    if case.get("oracle"):
        refs = [oracle.OracleGenerator(n, oracle.default_settings(**_case_settings(case, c))) for c in range(cascades)]
    for k, (dt, update) in enumerate(FRAMES):
        gens = [full] + [g for _, _, g in budgeted]
        if update:
            for g in gens:
                ocean.apply_settings(g.GetOceanSettings(0), U_10=25.0)
            for r in refs[:1]:
                r.settings.U_10 = 25.0
        for g in gens:
            g.CalculateOcean(dt, update_ocean=update)
        for r in refs:
            r.calculate_ocean(dt, update_ocean=update)
        h0_ptrs = None
        if k in (0, 2):  # the getter materialises h0 after a fused re-seed, on each plan's own grid
            h0_ptrs = {id(g): [g.GetInitialSpectrum(c) for c in range(cascades)] for g in gens}
        for g in gens:
            g.fft.synchronize()
        for b, _, gen in budgeted:
            for c in range(cascades):
                for (name, p_full, nb), (_, p_bud, _) in zip(_map_ptrs(full, c), _map_ptrs(gen, c)):
                    assert _same_on_device(p_full, p_bud, nb), (case["id"], "budget", b, "frame", k, "cascade", c, name)
                if h0_ptrs:
                    assert _same_on_device(h0_ptrs[id(full)][c], h0_ptrs[id(gen)][c], n * n * 16), \
                        (case["id"], "budget", b, "frame", k, "cascade", c, "h0")
    if refs:
        _, _, gen = budgeted[0]
        for c in (range(cascades) if cascades <= 3 else (0, 1, cascades // 2, cascades - 1)):
            assert gen.GetOceanSettings(c).time == refs[c].settings.time
            _frame_check(gen.height_map_host(c), gen.displacement_map_host(c), gen.jacobian_map_host(c), refs[c])
    for _, fft, gen in budgeted + [(0, full_fft, full)]:
        gen.close()
        fft.close()


@gpu
def test_sixty_four_cascades_under_budget_one(ocean):
    """OCEAN_MAX_CASCADES cascades of 64^2 on one CU's workgroups (k_cols_evolve<6>: 256 items, k_rows_final<6>:
    512, at most 32 workgroups): every cascade equals the same cascade computed alone on the full device."""
    n = 64
    for name, wg, items in full_kernels(n, 64):
        assert bound_holds(wg, items, 1), (name, wg, items)
    fft = ocean.FFTCalculator(n)
    fft.set_cu_budget(1)
    gen = ocean.Generator(fft, 64)
    for c in range(64):
        ocean.apply_settings(gen.GetOceanSettings(c), planeSize=3.0 + 7.0 * c, seed=(100 + c, 7 * c))
        for _, ptr, nb in _map_ptrs(gen, c):
            _fill_sentinel(ptr, nb)
    gen.CalculateOcean(0.5)
    one_fft = ocean.FFTCalculator(n)
    for c in range(64):
        one = ocean.Generator(one_fft, 1)
        ocean.apply_settings(one.GetOceanSettings(0), planeSize=3.0 + 7.0 * c, seed=(100 + c, 7 * c))
        one.CalculateOcean(0.5)
        assert np.array_equal(gen.height_map_host(c), one.height_map_host(0)), c
        assert np.array_equal(gen.displacement_map_host(c), one.displacement_map_host(0)), c
        assert np.array_equal(gen.jacobian_map_host(c), one.jacobian_map_host(0)), c
        one.close()


# ---- calculate_rates ---------------------------------------------------------------------------------
# k_rates_pack: 256-thread items. <true> (N >= 64): items = cascades * N^2 / 1024; <false> (N < 64): cascades *
# N^2 / 256. The batched EncodeIFFT of the 2 * cascades packed images follows (k_rows_ifft, k_cols).
RATE_CASES = [
    dict(id="rates-32x8", n=32, cascades=8, budgets=(1,), items=8 * 32 * 32 // 256),          # <false>: 256-texel tiles
    dict(id="rates-64x8", n=64, cascades=8, budgets=(1,), items=8 * 64 * 64 // 1024),        # 32 items >= 24
    dict(id="rates-1024x1", n=1024, cascades=1, budgets=(1, 32), items=1024 * 1024 // 1024),  # 1024 >= 768
]


@gpu
@pytest.mark.parametrize("case", RATE_CASES, ids=[c["id"] for c in RATE_CASES])
def test_budgeted_rates_equal_full_device(ocean, case):
    """ocean_generator_calculate_rates under a budget against the full device, bit for bit, on sentinel-filled
    rate maps; N = 64 also against tests/rates_ref.py at the gate of test_rate_maps_against_reference."""
    import rates_ref
    from oceansimulation_amd import capi
    from parity import channel_err

    L = capi.lib()
    n, cascades = case["n"], case["cascades"]
    for b in case["budgets"]:
        assert bound_holds(256, case["items"], b), (case["id"], b)
    gens = []
    for b in (0,) + case["budgets"]:
        fft = ocean.FFTCalculator(n)
        gen = ocean.Generator(fft, cascades)
        for c in range(cascades):
            ocean.apply_settings(gen.GetOceanSettings(c), planeSize=PLANE, seed=(12342 + 4097 * c, 8934))
        gen.CalculateOcean(1.0)
        gen.calculate_rates()  # allocates the rate maps
        fft.synchronize()
        if b:
            for c in range(cascades):
                _fill_sentinel(L.ocean_generator_height_rate_map(gen.handle, c), n * n * 16)
                _fill_sentinel(L.ocean_generator_displacement_rate_map(gen.handle, c), n * n * 16)
            fft.set_cu_budget(b)
            gen.calculate_rates()
            fft.synchronize()
        gens.append((b, fft, gen))
    _, _, full = gens[0]
    for b, _, gen in gens[1:]:
        for c in range(cascades):
            assert np.array_equal(gen.height_rate_map_host(c), full.height_rate_map_host(c)), (case["id"], b, c)
            assert np.array_equal(gen.displacement_rate_map_host(c), full.displacement_rate_map_host(c)), (case["id"], b, c)
    if n == 64:
        _, _, gen = gens[1]
        for c in range(cascades):
            s = R.settings_dict(gen.GetOceanSettings(c))
            rh, rd = rates_ref.rate_maps(s, n, gen.initial_spectrum_host(c))
            errs = channel_err(gen.height_rate_map_host(c), rh) + channel_err(gen.displacement_rate_map_host(c), rd)
            print(f"budget 1, cascade {c}: " + " ".join(f"{e:.2e}" for e in errs))
            assert max(errs) <= FRAME_TOL_GPU, (c, errs)


# ---- slabs -------------------------------------------------------------------------------------------
# Strip-dealt half-spectrum slabs: k_cols_half<ColsSlab> (256 / 512 threads, S strips per rank),
# k_half_to_rows (its grid is budget * 4 once tiles >= that), k_rows_half on row-major fields (w / 2 items).
SLAB_CASES = [dict(n=1024, ranks=2), dict(n=2048, ranks=4)]
SLAB_BUDGETS = (1, 3)


def _slab_frames(ocean, n, ranks, steps, settings, budget):
    """test_gpu_parity._slab_run on a plan with a budget, the maps and the exchange buffers sentinel-filled."""
    from oceansimulation_amd import capi
    from oceansimulation_amd.hip import DeviceBuffer
    from oceansimulation_amd.slab import SlabGenerator, emulate_frame

    L = capi.lib()
    fft = ocean.FFTCalculator(n)
    fft.set_cu_budget(budget)
    slabs = [SlabGenerator(fft, r, ranks) for r in range(ranks)]
    for g in slabs:
        ocean.apply_settings(g.GetOceanSettings(), **settings)
        rows = n // ranks
        _fill_sentinel(L.ocean_generator_height_map(g.handle, 0), rows * n * 16)
        _fill_sentinel(L.ocean_generator_displacement_map(g.handle, 0), rows * n * 16)
        _fill_sentinel(L.ocean_generator_jacobian_map(g.handle, 0), rows * n * 4)
    sends = [DeviceBuffer(g.exchange_bytes) for g in slabs]
    recvs = [DeviceBuffer(g.exchange_bytes) for g in slabs]
    for buf in sends + recvs:
        _fill_sentinel(buf.ptr, buf.nbytes)
    for k, dt in enumerate(steps):
        emulate_frame(slabs, sends, recvs, dt, update_ocean=(k == 0))
    out = tuple(np.concatenate([getattr(g, get)() for g in slabs])
                for get in ("height_map_host", "displacement_map_host", "jacobian_map_host"))
    for g in slabs:
        g.close()
    fft.close()
    return out


@gpu
@pytest.mark.parametrize("case", SLAB_CASES, ids=[f"{c['n']}x{c['ranks']}" for c in SLAB_CASES])
def test_budgeted_slabs_equal_whole_grid(ocean, case):
    """Slab frames with budgets 1 and 3 on the plan against the full-device whole grid, bit for bit."""
    n, ranks = case["n"], case["ranks"]
    k = col_first_cfg(n)
    strips = n // (2 * k["B"]) + 1
    per_rank = -(-strips // ranks)
    for b in SLAB_BUDGETS:
        # launch_half_slab_rows: tgrid = tiles < cus * 4 ? tiles : cus * 4
        assert half_to_rows_tiles(n, 1, ranks) >= 3 * b * 4, (n, ranks, b)
        assert bound_holds(k["T"] * 2, (n // ranks) // 2, b)  # k_rows_half on row-major fields
    assert bound_holds(k["T"] * k["B"], per_rank, 1)  # ColsSlab, budget 1
    settings, steps = dict(planeSize=PLANE), [0.25, 1.0 / 60.0]
    fft = ocean.FFTCalculator(n)
    gen = ocean.Generator(fft, 1)
    ocean.apply_settings(gen.GetOceanSettings(0), **settings)
    for dt in steps:
        gen.CalculateOcean(dt)
    want = (gen.height_map_host(0), gen.displacement_map_host(0), gen.jacobian_map_host(0))
    for b in SLAB_BUDGETS:
        got = _slab_frames(ocean, n, ranks, steps, settings, b)
        for name, g, w in zip(("height", "displacement", "jacobian"), got, want):
            assert np.array_equal(g, w), (n, ranks, "budget", b, name)


# ---- hull sets ---------------------------------------------------------------------------------------
# k_hulls_loads: one wave (64 threads) per tile of <= 64 points, so items >= instance points / 64;
# k_hulls_fold: 256 threads per body with more than one tile.
HULL_CASES = [
    dict(id="300x70", bodies=300, points=70, folds=300, reference=True),   # two tiles per body: the fold launch
    dict(id="4096x16", bodies=4096, points=16, folds=0, reference=False),  # four bodies share a wave
]


@pytest.fixture(scope="module")
def hull_scene(ocean):
    """Three 64^2 cascades with their rates on one plan: (plan, sampler, host maps, host rate maps)."""
    from oceansimulation_amd.surface import SurfaceSampler, host_cascades

    fft = ocean.FFTCalculator(64)
    gens = []
    for plane in (5.0, 17.0, 101.0):
        g = ocean.Generator(fft, 1)
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=plane)
        g.CalculateOcean(1.0)
        g.calculate_rates()
        gens.append(g)
    pairs = [(g, 0) for g in gens]
    rates = [(g.height_rate_map_host(0), g.displacement_rate_map_host(0)) for g in gens]
    return fft, SurfaceSampler(pairs), host_cascades(pairs), rates, gens


def _hull_loads(hulls, sampler, poses, velocity):
    """HullSet.loads_host with sentinel-filled outputs."""
    from oceansimulation_amd.hip import DeviceBuffer

    src = DeviceBuffer.from_array(poses)
    out = DeviceBuffer(hulls.bodies * 32)
    pts = DeviceBuffer(hulls.instance_points * 32)
    _fill_sentinel(out.ptr, out.nbytes)
    _fill_sentinel(pts.ptr, pts.nbytes)
    hulls.loads(sampler, src.ptr, out.ptr, pts.ptr, 9810.0, 8, 0.0, velocity)
    hulls.fft.synchronize()
    return out.to_host((hulls.bodies, 8)), pts.to_host((hulls.instance_points, 8))


@gpu
@pytest.mark.parametrize("velocity", [False, True])
@pytest.mark.parametrize("case", HULL_CASES, ids=[c["id"] for c in HULL_CASES])
def test_budgeted_hull_loads_equal_full_device(ocean, oracle, hull_scene, case, velocity):
    """ocean_hulls_loads at budget 1 against budget 0 on the same plan, bit for bit (the sum order is part of
    the contract); 300 x 70 at budget 1 also against tests/hull_loads_ref.py."""
    import hull_loads_ref as H
    from oceansimulation_amd.surface import HullSet
    from test_hulls import _random_points, _random_poses

    fft, sampler, host, rates, _ = hull_scene
    rng = np.random.default_rng(case["bodies"])
    points = _random_points(rng, case["points"])
    ranges = np.tile(np.array([[0, case["points"]]], np.int32), (case["bodies"], 1))
    poses = _random_poses(rng, case["bodies"])
    hulls = HullSet(fft, points, ranges)
    assert hulls.instance_points == case["bodies"] * case["points"]
    assert bound_holds(64, -(-hulls.instance_points // 64), 1)
    if case["folds"]:
        assert case["points"] > 64 and bound_holds(256, case["folds"], 1)
    try:
        full = _hull_loads(hulls, sampler, poses, velocity)
        fft.set_cu_budget(1)
        one = _hull_loads(hulls, sampler, poses, velocity)
    finally:
        fft.set_cu_budget(0)
    assert np.array_equal(one[0], full[0]) and np.array_equal(one[1], full[1])
    assert np.all(one[0][:, 7] >= 0.0)
    if case["reference"]:
        want_loads, want_pts, _ = H.hull_loads(oracle, host, rates, points, ranges, poses, 9810.0, 8, 0.0, velocity)
        assert np.array_equal(one[1], want_pts) and np.array_equal(one[0], want_loads)
    hulls.close()


# ---- the surface consumer's point kernels -------------------------------------------------------------
# launch_surface.hip: k_surface, k_surface_query, k_surface_velocity and k_surface_lod run one thread per point
# on at most budget * 8 workgroups of 256 (launch_points), k_surface_atlas one per map texel on at most budget * 4.
POINT_BUDGETS = (1, 3)
POINTS = 24576


def query_uses_atlas(cascades, n, points, iterations):
    """surface_query_use_atlas (launch_surface.hip), restated."""
    texels = 2 * cascades * n * n
    floor_points, per_point = (16384, 96) if iterations >= 2 else (65536, 48)
    return points >= floor_points and points * per_point >= texels and texels * 16 <= 256 << 20


@gpu
def test_budgeted_point_kernels_equal_full_device(ocean, hull_scene):
    """ocean_surface_sample, _query (8 iterations: the atlas repack and k_surface_query<true>; 1 iteration:
    <false>), _velocity and _sample_lod (footprints from below level 0 to past the top level) on 24576 points
    of three 64^2 cascades at budgets 1 and 3 against budget 0 on the same plan, bit for bit, every output
    filled with 0xFF bytes first. Each request is compared with itself only."""
    from oceansimulation_amd.hip import DeviceBuffer

    fft, sampler, _, _, gens = hull_scene
    n, cascades = 64, len(gens)
    for b in POINT_BUDGETS:
        assert POINTS >= 3 * 8 * 256 * b + 1       # every thread of the four point kernels runs >= 3 items
        assert cascades * n * n >= 3 * 4 * 256 * b  # and every thread of the repack
    assert query_uses_atlas(cascades, n, POINTS, 8) and not query_uses_atlas(cascades, n, POINTS, 1)
    for g in gens:
        g.build_mips()
    rng = np.random.default_rng(17)
    xz = rng.uniform(-150.0, 150.0, (POINTS, 2)).astype(np.float32)
    footprint = np.exp(rng.uniform(np.log(0.01), np.log(200.0), POINTS)).astype(np.float32)
    for plane in (5.0, 101.0):  # r = footprint * N / planeSize: below 1 (level 0 alone) up to >= N (the top level)
        r = footprint * np.float32(n) / np.float32(plane)
        assert r.min() < 1.0 and r.max() >= n / 2
    assert (footprint * np.float32(n) / np.float32(5.0)).max() >= n
    xz_dev = DeviceBuffer.from_array(xz)
    xzf_dev = DeviceBuffer.from_array(np.concatenate([xz, footprint[:, None]], axis=1))
    out = DeviceBuffer(POINTS * 32)
    calls = {
        "sample": lambda: sampler.sample(xz_dev.ptr, POINTS, out.ptr),
        "query-8": lambda: sampler.query(xz_dev.ptr, POINTS, 8, 0.0, out.ptr),
        "query-1": lambda: sampler.query(xz_dev.ptr, POINTS, 1, 0.0, out.ptr),
        "velocity": lambda: sampler.velocity(xz_dev.ptr, POINTS, out.ptr),
        "sample_lod": lambda: sampler.sample_lod(xzf_dev.ptr, POINTS, out.ptr),
    }

    def run(budget):
        got = {}
        fft.set_cu_budget(budget)
        for name, call in calls.items():
            _fill_sentinel(out.ptr, out.nbytes)
            call()
            fft.synchronize()
            got[name] = out.to_host((POINTS, 8)).view(np.uint32)
        return got

    try:
        full = run(0)
        budgeted = {b: run(b) for b in POINT_BUDGETS}
    finally:
        fft.set_cu_budget(0)
    for name, want in full.items():
        assert not (want == 0xFFFFFFFF).all(axis=1).any(), name  # no point left unwritten
        for b in POINT_BUDGETS:
            assert np.array_equal(budgeted[b][name], want), (name, "budget", b)
    for buf in (xz_dev, xzf_dev, out):
        buf.free()
