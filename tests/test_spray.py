"""Spray emitters: ocean_spray_emit and its counts against the contract restated in numpy float32
(tests/spray_ref.py, on rates_ref for the records' positions and velocities).

Scene: test_foam.py's, WaveApp's three cascades (planes 5 / 17 / 101 m), default settings, eight frames of
CalculateOcean(0.25, first frame only: update). The CPU tests pin the restatement on the oracle's maps (N = 64); the
GPU tests compare the kernels with the restatement evaluated on the GPU's own Jacobian maps, bit for bit: the
contract fixes every rounding and the order of the list, so there is no tolerance. Every output buffer is filled
with 0xFF bytes before a call.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rates_ref
import spray_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (5.0, 17.0, 101.0)
DT = 0.25
FRAMES = 8
SEED, STEP = 12345, 7
ALL = 1e30  # a rate at which every breaking texel emits
NEW_CALLS = ("ocean_default_spray_settings", "ocean_spray_create", "ocean_spray_destroy", "ocean_spray_emit",
             "ocean_spray_counts", "ocean_spray_counts_device")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _settings(threshold, rates, seed=SEED):
    rates = rates if isinstance(rates, (tuple, list)) else (rates,) * len(PLANES)
    return [(threshold, r, seed) for r in rates]


# ---- without a GPU ----------------------------------------------------------------------------
def test_exports_and_signatures():
    from oceansimulation_amd import capi
    import oceansimulation_amd as ocean
    from oceansimulation_amd import surface

    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    for name in ("emit", "emit_host", "counts", "counts_device", "close"):
        assert hasattr(ocean.SprayEmitter, name), name
    assert ocean.SprayEmitter is surface.SprayEmitter and "SprayEmitter" in surface.__all__
    assert hasattr(ocean, "apply_spray_settings") and hasattr(ocean, "default_spray_settings")
    assert hasattr(ocean, "OceanSpraySettings")


def test_default_spray_settings_and_size():
    from oceansimulation_amd import capi
    import oceansimulation_amd as ocean

    assert ctypes.sizeof(capi.OceanSpraySettings) == 12
    s = capi.OceanSpraySettings(-1.0, -1.0, 99)
    capi.lib().ocean_default_spray_settings(ctypes.byref(s))
    assert (s.threshold, s.rate, s.seed) == (np.float32(0.9), 8.0, 0)
    capi.lib().ocean_default_spray_settings(None)  # a null output is ignored
    s = ocean.default_spray_settings(rate=64.0, seed=5)
    assert (s.threshold, s.rate, s.seed) == (np.float32(0.9), 64.0, 5)
    with pytest.raises(AttributeError):
        ocean.apply_spray_settings(s, gain=1.0)
    header = open(os.path.join(ROOT, "include", "oceanfft.h")).read()
    body = header[header.index("typedef struct ocean_spray_settings"):header.index("} ocean_spray_settings;")]
    order = sorted(("threshold", "rate", "seed"), key=lambda f: body.index(f" {f};"))
    assert order == [f[0] for f in capi.OceanSpraySettings._fields_]
    assert "float threshold;" in body and "float rate;" in body and "uint32_t seed;" in body


def test_rejected_arguments_name_the_call():
    """Everything that can be refused without a generator: OCEAN_ERR_INVALID (or a null pointer) with the entry
    point's name in ocean_last_error. The emitter is created on a plan pointer that is never dereferenced: no
    call gets as far as the device."""
    from oceansimulation_amd import capi

    L = capi.lib()
    inv = capi.OCEAN_ERR_INVALID
    one = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
    h = ctypes.c_void_p()
    assert L.ocean_spray_create(None, one) == inv and b"ocean_spray_create" in L.ocean_last_error()
    assert L.ocean_spray_create(ctypes.byref(h), None) == inv and b"ocean_spray_create" in L.ocean_last_error()
    assert L.ocean_spray_create(ctypes.byref(h), one) == capi.OCEAN_OK and h
    counts = (ctypes.c_int64 * 18)()
    assert L.ocean_spray_counts(None, counts) == inv and b"ocean_spray_counts: null emitter" in L.ocean_last_error()
    assert L.ocean_spray_counts(h, counts) == inv and b"ocean_spray_counts: the emitter has no counts" in L.ocean_last_error()
    assert not L.ocean_spray_counts_device(None) and b"ocean_spray_counts_device" in L.ocean_last_error()
    assert not L.ocean_spray_counts_device(h) and b"ocean_spray_counts_device" in L.ocean_last_error()

    g1, c1 = (ctypes.c_void_p * 1)(None), (ctypes.c_int * 1)(0)
    g17, c17 = (ctypes.c_void_p * 17)(*([16] * 17)), (ctypes.c_int * 17)()
    good = (capi.OceanSpraySettings * 17)(*[capi.OceanSpraySettings(1.0, 8.0, 0) for _ in range(17)])

    def emit(spray=h, gens=g1, cas=c1, count=1, settings=good, dt=DT, capacity=4, out=one):
        return L.ocean_spray_emit(spray, gens, cas, count, settings, None, ctypes.c_float(dt), ctypes.c_uint32(STEP), 1,
                                  ctypes.c_int64(capacity), out)

    def one_setting(threshold, rate):
        return (capi.OceanSpraySettings * 1)(capi.OceanSpraySettings(threshold, rate, 0))

    nan, inf = float("nan"), float("inf")
    cases = [(dict(spray=None), b"null emitter"), (dict(gens=None), b"pairs"), (dict(cas=None), b"pairs"),
             (dict(count=0), b"pairs"), (dict(gens=g17, cas=c17, count=17), b"pairs"),
             (dict(settings=None), b"null settings"), (dict(capacity=-1), b"capacity"),
             (dict(out=None), b"capacity"), (dict(dt=-0.1), b"dt must be finite and >= 0"),
             (dict(dt=nan), b"dt must be finite and >= 0"), (dict(dt=inf), b"dt must be finite and >= 0"),
             (dict(settings=one_setting(nan, 8.0)), b"pair 0 has a non-finite threshold"),
             (dict(settings=one_setting(inf, 8.0)), b"pair 0 has a non-finite threshold"),
             (dict(settings=one_setting(1.0, -1.0)), b"pair 0 needs a rate"),
             (dict(settings=one_setting(1.0, inf)), b"pair 0 needs a rate"),
             (dict(settings=one_setting(1.0, nan)), b"pair 0 needs a rate"),
             (dict(), b"null generator")]
    for kwargs, word in cases:
        assert emit(**kwargs) == inv, (kwargs, word)
        assert b"ocean_spray_emit:" in L.ocean_last_error() and word in L.ocean_last_error(), L.ocean_last_error()
    assert L.ocean_spray_counts(h, counts) == inv  # refused calls allocate nothing
    assert L.ocean_spray_destroy(h) == capi.OCEAN_OK and L.ocean_spray_destroy(None) == capi.OCEAN_OK


def test_cpp_headers_compile_standalone(tmp_path):
    """A consumer of the spray emitter compiles against the drop-in headers alone."""
    src = tmp_path / "consumer.cpp"
    src.write_text(
        '#include "waves/Surface.h"\n'
        "#include <vector>\n"
        "Vision::ID frame(Waves::SprayEmitter& e, std::vector<Waves::Generator*>& gens, float dt, uint32_t step,\n"
        "                 int64_t* counts) {\n"
        "  std::vector<ocean_spray_settings> s(gens.size());\n"
        "  for (auto& v : s) { ocean_default_spray_settings(&v); v.rate = 64.0f; }\n"
        "  for (auto* g : gens) { g->CalculateOcean(dt); g->CalculateRates(); }\n"
        "  Vision::ID records = e.Emit(gens, s.data(), nullptr, dt, step, true, 65536);\n"
        "  e.GetCounts(counts);\n"
        "  const int64_t* table = e.GetCountsDevice(); (void)table;\n"
        "  return records;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}/include", "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    so = os.path.join(ROOT, "oceansimulation_amd", "libwaves.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", so], capture_output=True, text=True).stdout
    for sig in ("Waves::SprayEmitter::SprayEmitter(Vision::RenderDevice*, Waves::FFTCalculator*)",
                "Waves::SprayEmitter::~SprayEmitter()", "Waves::SprayEmitter::Emit(",
                "Waves::SprayEmitter::GetCounts(long*) const", "Waves::SprayEmitter::GetCountsDevice() const"):
        assert sig in syms, sig


@pytest.fixture(scope="module")
def cpu_jacs(oracle):
    """The Jacobian maps of the eighth frame on the oracle, N = 64."""
    gens = [oracle.OracleGenerator(64, oracle.default_settings(planeSize=L)) for L in PLANES]
    for k in range(FRAMES):
        for g in gens:
            g.calculate_ocean(DT, k == 0)
    return [np.array(g.jac, np.float32) for g in gens]


def test_reference_population(cpu_jacs):
    """Every arm of the predicate is populated at threshold 1.0: about half of the texels break, rate 64 thins
    them, and at threshold 0.9 the 101 m cascade has nothing to emit (the empty pair)."""
    nn = 64 * 64
    every = SR.emit(cpu_jacs, PLANES, _settings(1.0, ALL), DT, STEP)[3]
    some = SR.emit(cpu_jacs, PLANES, _settings(1.0, 64.0), DT, STEP)[3]
    steep = SR.emit(cpu_jacs, PLANES, _settings(0.9, ALL), DT, STEP)[3]
    print("found per pair: rate 1e30", every[2:5], "rate 64", some[2:5], "threshold 0.9", steep[2:5])
    for c in range(3):
        assert 0.25 * nn <= every[2 + c] <= 0.75 * nn, (c, every)
        assert every[2 + c] == np.count_nonzero(cpu_jacs[c] < np.float32(1.0))
        assert 100 <= some[2 + c] <= every[2 + c], (c, some)
    assert steep[2 + 2] == 0 and steep[2 + 0] >= 50, steep
    for counts in (every, some, steep):
        assert counts[0] == counts[1] == counts[2:].sum() and not counts[5:].any()


def test_reference_thinning_is_unbiased(cpu_jacs):
    """found against its expectation sum(p) within five standard deviations of the sum of independent Bernoulli
    draws, per pair, for several (seed, step) and two rates."""
    worst = 0.0
    for seed, step in ((12345, 7), (12345, 8), (1, 0), (0, 0), (99, 100000)):
        for rate in (8.0, 64.0):
            for c, jac in enumerate(cpu_jacs):
                emits, _, p = SR.predicate(jac, 1.0, rate, seed, DT, step)
                p = p.astype(np.float64)
                mean, sigma = p.sum(), np.sqrt((p * (1.0 - p)).sum())
                found = np.count_nonzero(emits)
                worst = max(worst, abs(found - mean) / sigma)
                assert abs(found - mean) <= 5.0 * sigma, (seed, step, rate, c, found, mean, sigma)
    print(f"worst deviation {worst:.2f} sigma")


def test_reference_steps_differ_and_order_is_nonzero_order(cpu_jacs):
    a = SR.emit(cpu_jacs, PLANES, _settings(1.0, 64.0), DT, 7)
    b = SR.emit(cpu_jacs, PLANES, _settings(1.0, 64.0), DT, 8)
    assert not np.array_equal(a[0], b[0])
    for c in range(3):  # each pair's set changes, not only the list
        assert set(a[0][a[0] >> 28 == c]) != set(b[0][b[0] >> 28 == c])
    ids, ds, base, counts = a
    want = []
    for c, jac in enumerate(cpu_jacs):
        emits, d, _ = SR.predicate(jac, 1.0, 64.0, SEED, DT, 7)
        y, x = np.nonzero(emits)
        want.append((c << 28) | (y * 64 + x))
        assert np.array_equal(ds[ids >> 28 == c], d[y, x]) and (d[y, x] > 0).all()
        cell = np.float32(PLANES[c]) / np.float32(64)
        assert np.array_equal(base[ids >> 28 == c], np.stack([(x.astype(np.float32) + np.float32(0.5)) * cell,
                                                              (y.astype(np.float32) + np.float32(0.5)) * cell], -1))
    want = np.concatenate(want).astype(np.uint32)
    assert np.array_equal(ids, want) and np.all(np.diff(ids.astype(np.int64)) > 0)
    # a capacity cuts the counts, not the list; tiles shift the base points by whole planes
    assert SR.emit(cpu_jacs, PLANES, _settings(1.0, 64.0), DT, 7, capacity=10)[3][:2].tolist() == [10, counts[1]]
    shifted = SR.emit(cpu_jacs, PLANES, _settings(1.0, 64.0), DT, 7, tiles=((3, -2), (0, 1), (-1, 0)))[2]
    first = ids >> 28 == 0
    assert np.allclose(shifted[first] - base[first], [15.0, -10.0], atol=1e-4)


# ---- on the GPU -------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


class Scene:
    """One three-cascade generator after the eight frames, with rates, and the host copies the restatement
    reads: built once per N and left unchanged."""

    def __init__(self, ocean, n):
        from oceansimulation_amd.surface import SprayEmitter, SurfaceSampler, host_cascades

        self.n = n
        self.fft = ocean.FFTCalculator(n)
        self.gen = ocean.Generator(self.fft, len(PLANES))
        for c, L in enumerate(PLANES):
            ocean.apply_settings(self.gen.GetOceanSettings(c), planeSize=L)
        for k in range(FRAMES):
            self.gen.CalculateOcean(DT, k == 0)
        self.gen.calculate_rates()
        self.sampler = SurfaceSampler([(self.gen, c) for c in range(len(PLANES))])
        self.emitter = SprayEmitter(self.fft)
        self.host = host_cascades(self.sampler.pairs)
        self.jacs = [h[2] for h in self.host]
        self.rates = [(self.gen.height_rate_map_host(c), self.gen.displacement_rate_map_host(c))
                      for c in range(len(PLANES))]
        self._want = {}

    def want(self, threshold, rate):
        """The restatement's full list for (threshold, rate) at SEED, STEP, DT: (records, counts, base points),
        computed once."""
        key = (threshold, rate)
        if key not in self._want:
            ids, ds, base, counts = SR.emit(self.jacs, PLANES, _settings(threshold, rate), DT, STEP)
            rows = rates_ref.surface_velocity(self.host, self.rates, base)
            self._want[key] = (SR.records(ids, ds, rows), counts, base)
        return self._want[key]

    def emit(self, settings, capacity, dt=DT, step=STEP, velocity=True, tiles=None, pad=3):
        """One call into a 0xFF-filled buffer of capacity + pad records: (the whole buffer as uint32 rows,
        counts). capacity 0 passes a null output."""
        from oceansimulation_amd.hip import DeviceBuffer

        rows = capacity + pad
        out = DeviceBuffer.from_array(np.full(rows * 32, 0xFF, np.uint8))
        self.emitter.emit(self.sampler, [dict(threshold=t, rate=r, seed=s) for t, r, s in settings], dt, step,
                          out.ptr if capacity else 0, capacity, velocity, tiles)
        counts = self.emitter.counts()
        table = ocean_hip_to_host(self.emitter.counts_device())
        assert np.array_equal(table, counts)
        return out.to_host((rows, 8), np.uint32), counts


def ocean_hip_to_host(ptr):
    from oceansimulation_amd import hip

    return hip.to_host(ptr, (18,), np.int64)


@pytest.fixture(scope="module")
def scenes(ocean):
    built = {}

    def get(n):
        if n not in built:
            built[n] = Scene(ocean, n)
        return built[n]

    return get


def _check_call(got, counts, want_records, want_counts, capacity):
    """The first `written` records are the restatement's, everything after them is still the sentinel."""
    written = min(int(want_counts[1]), capacity)
    expect = want_counts.copy()
    expect[0] = written
    assert np.array_equal(counts, expect), (counts, expect)
    assert np.array_equal(got[:written], _bits(want_records[:written]))
    assert np.all(got[written:] == 0xFFFFFFFF)


@gpu
@pytest.mark.parametrize("rate", [ALL, 64.0])
@pytest.mark.parametrize("n", [16, 32, 64, 256, 1024])
def test_records_equal_restatement(scenes, n, rate):
    """N = 16: one predicated eighth of a 2048-texel item per pair; 32: half an item; 64: two items per pair; 256:
    96 items; 1024: 1536 items, two chunks of the scan's 1024. A counting-only call first, then a call with room
    for exactly `found` records: the records against the restatement on rates_ref.surface_velocity, and slots
    0-2 and 4-6 against ocean_surface_velocity run on the restated base points."""
    sc = scenes(n)
    want, want_counts, base = sc.want(1.0, rate)
    found = int(want_counts[1])
    print(f"N = {n}, rate {rate:g}: found per pair {want_counts[2:5]}")
    assert found > 0 and (want_counts[2:5] > 0).all()
    got, counts = sc.emit(_settings(1.0, rate), 0)
    _check_call(got, counts, want, want_counts, 0)
    got, counts = sc.emit(_settings(1.0, rate), found)
    _check_call(got, counts, want, want_counts, found)
    rows = got[:found].view(np.float32)
    assert (rows[:, 3] > 0).all()
    vel = _bits(sc.sampler.velocity_host(base))
    assert np.array_equal(got[:found][:, [0, 1, 2, 4, 5, 6]], vel[:, [0, 1, 2, 4, 5, 6]])
    ids = got[:found, 7]
    assert np.all(np.diff(ids.astype(np.int64)) > 0) and (ids >> 28).max() == 2


@gpu
def test_empty_tiles_and_empty_pair(scenes):
    """Threshold 0.9 on 3 x 256^2: the 101 m cascade has no texel to emit and the 5 m one has items without any."""
    sc = scenes(256)
    want, want_counts, _ = sc.want(0.9, ALL)
    print("found per pair", want_counts[2:5])
    got, counts = sc.emit(_settings(0.9, ALL), int(want_counts[1]))
    _check_call(got, counts, want, want_counts, int(want_counts[1]))
    assert counts[2 + 2] == 0 and counts[2 + 0] >= 1000, counts
    # Rate 0.02 at threshold 1.0: p is about 1e-3 at most, a few dozen emitters in all, fewer per pair than its
    # 32 items, so emitting pairs have items without an emitter between items with one.
    want, want_counts, _ = sc.want(1.0, 0.02)
    got, counts = sc.emit(_settings(1.0, 0.02), int(want_counts[1]))
    _check_call(got, counts, want, want_counts, int(want_counts[1]))
    ids = got[:int(counts[0]), 7]
    per_item = np.bincount((ids >> 28) * 32 + ((ids & 0x0FFFFFFF) >> 11), minlength=96)  # 32 items of 2048 per pair
    print("sparse: found per pair", counts[2:5], "items without an emitter",
          [int((per_item[32 * c:32 * c + 32] == 0).sum()) for c in range(3)])
    assert (per_item == 0).any() and (per_item > 0).any() and 0 < counts[1] < 96


@gpu
def test_capacity(scenes):
    """found, a cut inside pair 0's second item, inside pair 1's first item, exactly pair 0's count (the pair
    boundary), 1 and 0 with a null output, at N = 64 (two items per pair)."""
    sc = scenes(64)
    want, want_counts, _ = sc.want(1.0, ALL)
    found, first = int(want_counts[1]), int(want_counts[2])
    in_item0 = int(np.count_nonzero(sc.jacs[0].ravel()[:2048] < np.float32(1.0)))
    assert 0 < in_item0 < first
    for capacity in (found, in_item0 + 5, in_item0, first + 37, first, first - 1, first + 1, 1, 0, found + 100):
        got, counts = sc.emit(_settings(1.0, ALL), capacity)
        _check_call(got, counts, want, want_counts, capacity)


@gpu
def test_velocity_off_gives_the_vertex_stage(scenes):
    sc = scenes(64)
    want, want_counts, base = sc.want(1.0, 64.0)
    found = int(want_counts[1])
    got, counts = sc.emit(_settings(1.0, 64.0), found, velocity=False)
    assert np.array_equal(counts, want_counts)
    sample = _bits(sc.sampler.sample_host(base))
    assert np.array_equal(got[:found, :3], sample[:, :3]) and np.array_equal(got[:found, :3], _bits(want)[:, :3])
    assert np.all(got[:found, 4:7] == 0)  # +0
    assert np.array_equal(got[:found][:, [3, 7]], _bits(want)[:, [3, 7]]) and np.all(got[found:] == 0xFFFFFFFF)


@gpu
def test_tiles_shift_the_base_points(scenes):
    sc = scenes(64)
    tiles = ((3, -2), (0, 1), (-1, 0))
    ids, ds, base, want_counts = SR.emit(sc.jacs, PLANES, _settings(1.0, 64.0), DT, STEP, tiles=tiles)
    plain = sc.want(1.0, 64.0)[2]
    assert np.array_equal(ids, sc.want(1.0, 64.0)[0].view(np.uint32)[:, 7]) and not np.array_equal(base, plain)
    want = SR.records(ids, ds, rates_ref.surface_velocity(sc.host, sc.rates, base))
    found = int(want_counts[1])
    got, counts = sc.emit(_settings(1.0, 64.0), found, tiles=tiles)
    _check_call(got, counts, want, want_counts, found)
    assert np.array_equal(got[:found][:, [0, 1, 2, 4, 5, 6]], _bits(sc.sampler.velocity_host(base))[:, [0, 1, 2, 4, 5, 6]])


@gpu
def test_pair_with_rate_zero_is_left_out(scenes):
    sc = scenes(64)
    settings = _settings(1.0, (64.0, 0.0, ALL))
    ids, ds, base, want_counts = SR.emit(sc.jacs, PLANES, settings, DT, STEP)
    assert want_counts[3] == 0 and want_counts[2] > 0 and want_counts[4] > 0
    want = SR.records(ids, ds, rates_ref.surface_velocity(sc.host, sc.rates, base))
    found = int(want_counts[1])
    got, counts = sc.emit(settings, found)
    _check_call(got, counts, want, want_counts, found)
    pairs = got[:found, 7] >> 28
    assert not (pairs == 1).any() and np.all(np.diff(got[:found, 7].astype(np.int64)) > 0)
    # no emitting pair at all: two launches fewer, counts all zero
    got, counts = sc.emit(_settings(1.0, 0.0), 8)
    assert not counts.any() and np.all(got == 0xFFFFFFFF)


@gpu
def test_replay_and_next_step(scenes):
    sc = scenes(256)
    found = int(sc.want(1.0, 64.0)[1][1])
    a, ca = sc.emit(_settings(1.0, 64.0), found)
    b, cb = sc.emit(_settings(1.0, 64.0), found)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    c, cc = sc.emit(_settings(1.0, 64.0), found, step=STEP + 1)
    ids, ds, base, want_counts = SR.emit(sc.jacs, PLANES, _settings(1.0, 64.0), DT, STEP + 1, capacity=found)
    assert np.array_equal(cc, want_counts)
    written = int(cc[0])
    assert np.array_equal(c[:written, 7], ids[:written]) and set(c[:written, 7]) != set(a[:found, 7])
    # another seed is another set as well
    d, cd = sc.emit(_settings(1.0, 64.0, seed=SEED + 1), found)
    assert set(d[:int(cd[0]), 7]) != set(a[:found, 7])


@gpu
def test_refusals(ocean, scenes):
    from oceansimulation_amd import capi
    from oceansimulation_amd.surface import SprayEmitter, SurfaceSampler

    sc = scenes(64)
    fresh = SprayEmitter(sc.fft)
    with pytest.raises(capi.OceanError, match="ocean_spray_counts: the emitter has no counts"):
        fresh.counts()
    with pytest.raises(capi.OceanError, match="ocean_spray_counts_device"):
        fresh.counts_device()
    gens = [ocean.Generator(sc.fft, 1) for _ in PLANES]
    for g, L in zip(gens, PLANES):
        ocean.apply_settings(g.GetOceanSettings(0), planeSize=L)
    sampler = SurfaceSampler([(g, 0) for g in gens])
    args = (sampler, dict(threshold=1.0, rate=64.0), DT, STEP)
    for g in gens[:2]:
        g.CalculateOcean(DT)
    with pytest.raises(capi.OceanError, match="ocean_spray_emit: generator 2 has no frame"):
        fresh.emit(*args)
    gens[2].CalculateOcean(DT)
    with pytest.raises(capi.OceanError, match="ocean_spray_emit: generator 0 has no rates"):
        fresh.emit(*args)
    fresh.emit(*args, velocity=False)  # counting needs no rates
    counted = fresh.counts()
    for g in gens:
        g.calculate_rates()
    fresh.emit(*args)
    assert np.array_equal(fresh.counts(), counted) and counted[1] > 0
    gens[1].CalculateOcean(DT)
    with pytest.raises(capi.OceanError, match="ocean_spray_emit: generator 1 has stale rates"):
        fresh.emit(*args)
    other = ocean.FFTCalculator(64)
    elsewhere = SprayEmitter(other)
    with pytest.raises(capi.OceanError, match="ocean_spray_emit: the first generator is on another plan than the emitter"):
        elsewhere.emit(*args, velocity=False)
    from oceansimulation_amd.slab import SlabGenerator
    slab1 = SlabGenerator(sc.fft, 0, 1)  # one rank: whole-grid sized, yet its maps are a slab pipeline's
    with pytest.raises(capi.OceanError,
                       match="ocean_spray_emit: generator 0 is a slab generator: row slabs, not whole maps"):
        fresh.emit(SurfaceSampler([(slab1, 0)]), dict(rate=1.0), DT, STEP, velocity=False)
    small = ocean.FFTCalculator(32)
    g32 = ocean.Generator(small, 1)
    g32.CalculateOcean(DT)
    with pytest.raises(capi.OceanError, match="ocean_spray_emit: all cascades must share one map size"):
        fresh.emit(SurfaceSampler([(gens[0], 0), (g32, 0)]), dict(rate=1.0), DT, STEP, velocity=False)
    elsewhere.close()
    fresh.close()
    for g in gens + [g32]:
        g.close()
    other.close()
    small.close()


# ---- the item loops under a CU budget ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [256, 1024])
def test_budgeted_call_equals_full_device(scenes, n):
    """k_spray_count / k_spray_scatter: 256 threads, items = 3 * N^2 / 2048 = 96 and 1536; under a budget of one CU
    the grid is at most 8 resident workgroups (tests/test_item_loops.py's bound: min(32, 2048 / 256) per CU), so
    every workgroup runs 12 or 192 items. k_spray_fill: at most 8 workgroups of 256 threads for more than 6144
    records. k_spray_scan's single workgroup does not depend on the budget. Records and counts bit for bit."""
    sc = scenes(n)
    want, want_counts, _ = sc.want(1.0, 64.0)
    found = int(want_counts[1])
    assert 3 * n * n // 2048 >= 3 * 8 and found >= 3 * 8 * 256 + 1
    results = []
    try:
        for budget in (0, 1):
            sc.fft.set_cu_budget(budget)
            results.append(sc.emit(_settings(1.0, 64.0), found))
    finally:
        sc.fft.set_cu_budget(0)
    _check_call(results[0][0], results[0][1], want, want_counts, found)
    assert np.array_equal(results[1][0], results[0][0]) and np.array_equal(results[1][1], results[0][1])
