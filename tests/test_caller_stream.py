"""The whole-grid API on a caller's non-blocking stream whose queue is still busy when each call returns.

include/oceanfft.h promises that every whole-grid call is enqueued on the stream given to ocean_fft_create, that
its outputs may be consumed by later work on that stream without a host wait, and that most calls do not wait for
the stream. Every other test creates its plans on the legacy null stream, which orders itself against every
blocking stream and against synchronous copies, and waits on the host between a call and the next read: a launch
on the wrong stream, a missing event edge to an internal stream, or a buffer freed under queued work cannot show
there. Here the plan's stream is created with hipStreamNonBlocking, and every sequence runs three times:

  reference  the sequence on a plan with stream 0 (what the other tests pin against numpy and the oracle), twice:
             the state a pass leaves (time, foam, the particle pool) is the next one's;
  cold       the first pass on the caller's stream, no stall: first-use allocations and occupancy queries;
  stalled    every output and library-owned product filled with 0xFF bytes, then on the stream: the stall (one
             ocean_debug_copy on one workgroup between two scratch buffers), event E, the copies that produce the
             device inputs from staging buffers into sentinel-filled input buffers, and the whole sequence with
             no host wait. E must still be pending when the last call has returned (a condition, not a
             measurement: it makes the case count, and it is the header's "no host synchronisation" under test).
             Then the stream is synchronised, every byte is compared with the reference's second pass, and no
             output may still hold the sentinel.

The reference passes fill the same sentinels at the same points, so the three runs differ in the stream alone.
Calls that the header documents as waiting (the *_counts and *_host readers, ocean_generator_bounds,
set_depth_layers with a changed count, the destroy calls) come after the final synchronise.

The stall, measured on an MI355X (profiles/caller_stream_stall.log): one workgroup copies 9.7 .. 16.0 GB/s
(16 MiB in 1.1 .. 1.7 ms, 64 MiB in 4.2 .. 6.3 ms, 128 MiB in 8.4 .. 11.1 ms, 256 MiB in 22 .. 28 ms). The host-side
issue of the longest sequences after their cold pass on the null-stream plan takes 0.25 .. 0.37 ms (frame overlap
at 1024, 37 calls with the per-frame copies), 0.31 .. 0.36 ms (the stateful chain, 30 calls) and 0.28 .. 0.42 ms
(the 42 interleaved calls of the two plans); the slowest issue of a stalled pass seen in four runs is 0.59 ms.
STALL_BYTES = 256 MiB: 16.8 ms at the fastest rate measured, 10 x 0.59 ms with a further factor of 2.8, and 0.2 s
only at 1.3 GB/s, a seventh of the slowest rate measured. The second plan of the two-plan test stalls for three
quarters of that, 12.6 ms >= 10 x 0.59 ms.
"""
import ctypes
import time

import numpy as np
import pytest

gpu = pytest.mark.gpu

MiB = 1 << 20
STALL_BYTES = 256 * MiB
PLANES = (5.0, 17.0, 101.0)
DEPTHS = (0.0, 0.25, 1.0, 4.0)
DEPTHS_8 = (0.0, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
CAMERA = (3.0, 12.0, -7.0, 0.6, 0.8)
FOAM = dict(bias=1.0, gain=32.0, decay=0.5, level=0.5)
DT = 0.25


@pytest.fixture(scope="module")
def ocean():
    import oceansimulation_amd as o
    from oceansimulation_amd import capi

    assert capi.lib().ocean_device_count() > 0, "no GPU visible to liboceanfft.so"
    return o


class Stall:
    """The two scratch buffers of the stall and the 0xFF source of the sentinel fills."""

    def __init__(self):
        from oceansimulation_amd.hip import DeviceBuffer

        self.a, self.b = DeviceBuffer(STALL_BYTES), DeviceBuffer(STALL_BYTES)
        self.ff = None

    def fill(self, ptr, nbytes):
        """0xFF over [ptr, ptr + nbytes), synchronous on the null stream; the caller synchronises the device."""
        from oceansimulation_amd import hip
        from oceansimulation_amd.hip import DeviceBuffer

        if self.ff is None or self.ff.nbytes < nbytes:
            hip.synchronize()
            self.ff = DeviceBuffer.from_array(np.full(max(nbytes, 16 * MiB), 0xFF, np.uint8))
        hip.copy_d2d(int(ptr), self.ff.ptr, nbytes)


@pytest.fixture(scope="module")
def stall():
    from oceansimulation_amd import hip

    s = Stall()
    yield s
    hip.synchronize()
    for b in (s.a, s.b, s.ff):
        if b is not None:
            b.free()


def _pad16(nbytes):
    return (nbytes + 15) // 16 * 16


class Seq:
    """A call sequence bound to one plan. calls(p) lists the thunks of pass p (0: cold, 1: the compared pass);
    products() lists (name, device pointer, bytes, mode) of every output and library-owned product (they exist
    after pass 0), mode being what "holds no sentinel" means for it: "words" no 32-bit word of 0xFF bytes, "rows"
    no 16-byte row of them, "some" not all of it (lists filled up to a device count, words that may be all ones);
    late() the host readers that wait for the stream."""

    def __init__(self, ocean, stream):
        self.ocean, self.stream = ocean, stream
        self.inputs, self.outs, self.held, self.kept = [], [], [], {}

    def input(self, arr):
        """A device input produced on the stream from a staging copy of arr; returns its pointer."""
        from oceansimulation_amd.hip import DeviceBuffer

        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint8)
        padded = np.zeros(_pad16(raw.size), np.uint8)
        padded[:raw.size] = raw
        dst, src = DeviceBuffer(padded.size), DeviceBuffer.from_array(padded)
        self.inputs.append((dst, src))
        return dst.ptr

    def output(self, name, nbytes, mode="rows"):
        from oceansimulation_amd.hip import DeviceBuffer

        buf = DeviceBuffer(nbytes)
        self.outs.append((name, buf.ptr, nbytes, mode))
        self.held.append(buf)
        return buf.ptr

    def keep(self, name, get_ptr, nbytes, mode="rows"):
        """A thunk that copies nbytes at get_ptr() into a buffer of the test's on the stream: later work on the same
        stream consuming an output with no host wait, and the only witness of a product that the sequence rewrites."""
        from oceansimulation_amd.waves import debug_copy

        if name not in self.kept:
            self.kept[name] = self.output(name, nbytes, mode)
        dst = self.kept[name]
        return lambda: debug_copy(dst, get_ptr(), nbytes, 64, self.stream)

    def keep_frames(self, thunks, gen, p):
        """thunks with a copy of every map of gen after each thunk marked as a frame."""
        out, k, n = [], 0, gen.n
        for t in thunks:
            out.append(t)
            if getattr(t, "is_frame", False):
                for c in range(gen.cascades):
                    out += [self.keep(f"frame{k}.height{c}", lambda c=c: gen.GetHeightMap(c), n * n * 16),
                            self.keep(f"frame{k}.displacement{c}", lambda c=c: gen.GetDisplacementMap(c), n * n * 16),
                            self.keep(f"frame{k}.jacobian{c}", lambda c=c: gen.GetJacobianMap(c), n * n * 4, "words")]
                k += 1
        return out

    def map_products(self, gen, prefix=""):
        n, out = gen.n, []
        for c in range(gen.cascades):
            out += [(f"{prefix}height{c}", gen.GetHeightMap(c), n * n * 16, "rows"),
                    (f"{prefix}displacement{c}", gen.GetDisplacementMap(c), n * n * 16, "rows"),
                    (f"{prefix}jacobian{c}", gen.GetJacobianMap(c), n * n * 4, "words")]
        return out

    def products(self):
        return list(self.outs)

    def late(self):
        return {}

    def close(self):
        for dst, src in self.inputs:
            dst.free()
            src.free()
        for b in self.held:
            b.free()


def frame(thunk):
    """Marks a thunk as a frame for Seq.keep_frames."""
    thunk.is_frame = True
    return thunk


def _sync(stream):
    from oceansimulation_amd import hip

    if stream:
        hip.stream_synchronize(stream)
    else:
        hip.synchronize()


def run_pass(seqs, p, stall, stall_bytes=(), probe=None):
    """One pass of the sequences (interleaved call by call when there are several): sentinels, the stalls and
    their events, the inputs, the calls; -> (snapshots, E pending after the last call returned, issue seconds)."""
    from oceansimulation_amd import hip
    from oceansimulation_amd.waves import debug_copy

    for q in seqs:
        _sync(q.stream)
    lists = [q.calls(p) for q in seqs]  # first: a list may create buffers of its own, which the fills below cover
    for q in seqs:  # pass 0 creates the library-owned products: only the test's own buffers exist before it
        for _, ptr, nbytes, _ in (q.products() if p > 0 else []) + q.outs:
            stall.fill(ptr, nbytes)
    for q in seqs:
        for dst, _ in q.inputs:
            stall.fill(dst.ptr, dst.nbytes)
    hip.synchronize()
    events = []
    for q, nbytes in zip(seqs, stall_bytes):
        assert nbytes <= STALL_BYTES and nbytes % 16 == 0
        debug_copy(stall.b.ptr, stall.a.ptr, nbytes, 1, q.stream)
        events.append(hip.event_create())
        hip.event_record(events[-1], q.stream)
    for q in seqs:
        for dst, src in q.inputs:
            debug_copy(dst.ptr, src.ptr, dst.nbytes, 4, q.stream)
    t0 = time.perf_counter()
    for k in range(max(len(l) for l in lists)):
        for l in lists:
            if k < len(l):
                l[k]()
    issue = time.perf_counter() - t0
    pending = [not hip.event_query(e) for e in events]
    seen = probe() if probe else None
    for q in seqs:
        _sync(q.stream)
    for e in events:
        assert hip.event_query(e)
        hip.event_destroy(e)
    snaps = []
    for q in seqs:
        snap = {name: (hip.to_host(ptr, (nbytes,), np.uint8), mode) for name, ptr, nbytes, mode in q.products()}
        for name, arr in (q.late() if p > 0 else {}).items():  # the getters touch state (the h0 memo): last pass only
            snap[name] = (np.ascontiguousarray(arr).view(np.uint8).reshape(-1), None)
        snaps.append(snap)
    return snaps, pending, issue, seen


def _same(got, want, label):
    assert sorted(got) == sorted(want), label
    for name, (arr, _) in got.items():
        assert np.array_equal(arr, want[name][0]), (label, name, int(np.count_nonzero(arr != want[name][0])))


def _no_sentinel(snap, label):
    for name, (arr, mode) in snap.items():
        if mode == "words":
            assert not (arr.view(np.uint32) == 0xFFFFFFFF).any(), (label, name)
        elif mode == "rows":
            assert not (arr.reshape(-1, 16) == 0xFF).all(axis=1).any(), (label, name)
        elif mode == "some":
            assert not (arr == 0xFF).all(), (label, name)


def check(ocean, stall, makers, stall_bytes=None, label=""):
    """The reference, cold and stalled passes of one sequence per maker, each on a non-blocking stream of its own."""
    from oceansimulation_amd import hip

    stall_bytes = stall_bytes or [STALL_BYTES] * len(makers)
    want = []
    refs = [make(ocean, 0) for make in makers]
    for p in range(2):
        snaps, _, issue, _ = run_pass(refs, p, stall)
        want.append(snaps)
    print(f"{label}: {sum(len(q.calls(1)) for q in refs)} calls issued in {1e3 * issue:.3f} ms on the null stream")
    for q in refs:
        _no_sentinel(want[1][refs.index(q)], label + " (null stream)")
        q.close()
    streams = [hip.stream_create(hip.STREAM_NON_BLOCKING) for _ in makers]
    seqs = []
    try:
        for s in streams:
            assert hip.stream_flags(s) & hip.STREAM_NON_BLOCKING
        seqs = [make(ocean, s) for make, s in zip(makers, streams)]
        cold, _, _, _ = run_pass(seqs, 0, stall)
        for k in range(len(seqs)):
            _same(cold[k], want[0][k], f"{label} cold {k}")
        got, pending, issue, _ = run_pass(seqs, 1, stall, stall_bytes)
        print(f"{label}: stalled pass issued in {1e3 * issue:.3f} ms, E pending {pending}")
        assert all(pending), (label, "the stall's event completed before the last call returned", pending, issue)
        for k in range(len(seqs)):
            _same(got[k], want[1][k], f"{label} stalled {k}")
            _no_sentinel(got[k], f"{label} stalled {k}")
    finally:
        for q in seqs:  # a plan goes before its stream does, after a failed comparison too
            q.close()
        hip.synchronize()
        for s in streams:
            hip.stream_destroy(s)


# ---- a. frames -----------------------------------------------------------------------------------------
class Frames64(Seq):
    """N = 64, three cascades, the full path: three frames, the second after a settings edit with update_spectrum."""

    def __init__(self, ocean, stream):
        super().__init__(ocean, stream)
        self.fft = ocean.FFTCalculator(64, stream=stream)
        self.gen = ocean.Generator(self.fft, 3)
        for c, plane in enumerate(PLANES):
            ocean.apply_settings(self.gen.GetOceanSettings(c), planeSize=plane)

    def calls(self, p):
        g = self.gen

        def edit():
            g.GetOceanSettings(1).U_10 = 20.0 + 5.0 * p

        return self.keep_frames([frame(lambda: g.CalculateOcean(DT, p == 0)), edit,
                                 frame(lambda: g.CalculateOcean(1.0 / 60.0, True)),
                                 frame(lambda: g.CalculateOcean(1.0 / 60.0))], g, p)

    def products(self):
        return self.map_products(self.gen) + list(self.outs)

    def late(self):
        return {f"h0_{c}": self.gen.initial_spectrum_host(c) for c in range(3)}

    def close(self):
        super().close()
        self.gen.close()
        self.fft.close()


class Frames1024(Seq):
    """N = 1024, one cascade, the blocked half path. Cold: the first seeding, both frame paths, frame overlap on.
    Compared: a memo-skipped re-seed, a fused re-seed after a U_10 edit, generate_spectrum between frames, frame
    overlap off and one more frame, set_half_spectrum(0 / 1) between frames."""

    overlap = False

    def __init__(self, ocean, stream):
        super().__init__(ocean, stream)
        self.fft = ocean.FFTCalculator(1024, stream=stream)
        self.gen = ocean.Generator(self.fft, 1)
        ocean.apply_settings(self.gen.GetOceanSettings(0), planeSize=40.0)

    def calls(self, p):
        g, dt = self.gen, 1.0 / 60.0

        def plain():
            return frame(lambda: g.CalculateOcean(dt))

        if p == 0:
            out = [frame(lambda: g.CalculateOcean(0.5, True)), lambda: g.set_half_spectrum(False), plain(),
                   lambda: g.set_half_spectrum(True), plain()]
            if self.overlap:
                out += [lambda: g.set_frame_overlap(True), plain(), plain()]
            return self.keep_frames(out, g, p)

        def edit():
            g.GetOceanSettings(0).U_10 = 25.0

        out = [frame(lambda: g.CalculateOcean(dt, True)), edit, frame(lambda: g.CalculateOcean(dt, True)), plain(),
               g.GenerateSpectrum, plain(), plain()]
        if self.overlap:
            out += [lambda: g.set_frame_overlap(False), plain()]
        out += [lambda: g.set_half_spectrum(False), plain(), lambda: g.set_half_spectrum(True), plain()]
        return self.keep_frames(out, g, p)

    def products(self):
        return self.map_products(self.gen) + list(self.outs)

    def late(self):
        return {"h0": self.gen.initial_spectrum_host(0)}

    def close(self):
        super().close()
        self.gen.close()
        self.fft.close()


class Frames1024Overlap(Frames1024):
    overlap = True


@gpu
@pytest.mark.parametrize("seq", [Frames64, Frames1024, Frames1024Overlap], ids=lambda s: s.__name__)
def test_frames(ocean, stall, seq):
    check(ocean, stall, [seq], label=seq.__name__)


# ---- b. derived products -------------------------------------------------------------------------------
class Derived(Seq):
    """Straight after a frame: build_mips, calculate_rates, set_depth_layers (same count) + calculate_kinematics,
    build_bounds, advance_foam twice, reset_foam, advance_foam. The cold pass first runs calculate_kinematics with
    8 layers after calculate_rates (the EncodeIFFT work image grows: a hipFree may wait) and goes back to 4."""

    n, cascades, planes, reseed = 64, 3, PLANES, False

    def __init__(self, ocean, stream):
        super().__init__(ocean, stream)
        self.fft = ocean.FFTCalculator(self.n, stream=stream)
        self.gen = g = ocean.Generator(self.fft, self.cascades)
        for c, plane in enumerate(self.planes):
            ocean.apply_settings(g.GetOceanSettings(c), planeSize=plane)
            ocean.apply_foam_settings(g.GetFoamSettings(c), **FOAM)

    def calls(self, p):
        g = self.gen
        out = []
        if p == 0:
            out += [lambda: g.CalculateOcean(0.5, True), g.calculate_rates, lambda: g.set_depth_layers(DEPTHS_8),
                    g.calculate_kinematics, lambda: g.set_depth_layers(DEPTHS)]
        if self.reseed:  # a fused re-seed: materialise_h0 writes h0 on the stream inside calculate_rates

            def edit():
                g.GetOceanSettings(0).U_10 = 25.0 + 5.0 * p

            out += [edit, lambda: g.CalculateOcean(DT, True)]
        else:
            out += [lambda: g.CalculateOcean(DT)]
        depths = tuple(d + 0.5 * p for d in DEPTHS)
        return out + [g.build_mips, g.calculate_rates, lambda: g.set_depth_layers(depths), g.calculate_kinematics,
                      g.build_bounds, lambda: g.advance_foam(DT), lambda: g.advance_foam(DT), g.reset_foam,
                      lambda: g.advance_foam(DT)]

    def products(self):
        from oceansimulation_amd import capi

        L, g, n = capi.lib(), self.gen, self.n
        out = self.map_products(g)
        for c in range(g.cascades):
            for level in range(1, g.mip_levels()):
                side = n >> level
                out += [(f"height_mip{c}.{level}", L.ocean_generator_height_mip(g.handle, c, level), side * side * 16, "rows"),
                        (f"displacement_mip{c}.{level}", L.ocean_generator_displacement_mip(g.handle, c, level),
                         side * side * 16, "rows"),
                        (f"jacobian_mip{c}.{level}", L.ocean_generator_jacobian_mip(g.handle, c, level), side * side * 4,
                         "words")]
            out += [(f"height_rate{c}", L.ocean_generator_height_rate_map(g.handle, c), n * n * 16, "rows"),
                    (f"displacement_rate{c}", L.ocean_generator_displacement_rate_map(g.handle, c), n * n * 16, "rows"),
                    (f"foam{c}", g.GetFoamMap(c), n * n * 4, "words")]
            for layer in range(len(DEPTHS)):
                for image in range(2):
                    out.append((f"kinematics{c}.{layer}.{image}", g.GetKinematicsMap(c, layer, image), n * n * 16, "rows"))
        out += [("bounds", L.ocean_generator_bounds_device(g.handle), g.cascades * 18 * 4, "words"),
                ("foam_counts", g.foam_counts_device(), g.cascades * 3 * 8, "some")]
        return out

    def late(self):
        g = self.gen
        out = {f"bounds_host{c}": g.GetBounds(c) for c in range(g.cascades)}
        out.update({f"foam_counts_host{c}": g.GetFoamCounts(c) for c in range(g.cascades)})
        out.update({f"h0_{c}": g.initial_spectrum_host(c) for c in range(g.cascades)})
        return out

    def close(self):
        super().close()
        self.gen.close()
        self.fft.close()


class Derived1024(Derived):
    n, cascades, planes, reseed = 1024, 1, (40.0,), True


@gpu
@pytest.mark.parametrize("seq", [Derived, Derived1024], ids=lambda s: s.__name__)
def test_derived_products(ocean, stall, seq):
    check(ocean, stall, [seq], label=seq.__name__)


# ---- c. point consumers --------------------------------------------------------------------------------
class Points(Derived):
    """The device-pointer entry points of surface.py after the products they read, every input produced on the
    stream: query with 70000 points (the atlas path), then 3000 on the same plan (the direct path beside the shared
    atlas buffer), sample, sample_plane, sample_lod, sample_plane_lod, velocity, kinematics, raycast, sample_foam,
    sample_plane_foam_device."""

    seed = 5

    def __init__(self, ocean, stream):
        from oceansimulation_amd.surface import SurfaceSampler
        from test_raycast import make_rays

        super().__init__(ocean, stream)
        rng = np.random.default_rng(self.seed)
        self.sampler = SurfaceSampler([(self.gen, c) for c in range(3)])
        self.many, self.few, self.res = 70000, 3000, 24
        xz_many = rng.uniform(-400.0, 400.0, (self.many, 2)).astype(np.float32)
        xz = rng.uniform(-150.0, 150.0, (self.few, 2)).astype(np.float32)
        footprint = np.exp(rng.uniform(np.log(0.01), np.log(200.0), self.few)).astype(np.float32)
        xyz = np.concatenate([xz[:, :1], rng.uniform(-6.0, 1.0, (self.few, 1)).astype(np.float32), xz[:, 1:]], axis=1)
        self.rays = 1024
        self.in_many, self.in_xz = self.input(xz_many), self.input(xz)
        self.in_xzf = self.input(np.concatenate([xz, footprint[:, None]], axis=1))
        self.in_xyz, self.in_rays = self.input(xyz), self.input(make_rays(self.rays))
        plane = (self.res + 1) ** 2
        self.o = {name: self.output(name, rows * width * 4) for name, rows, width in (
            ("query_atlas", self.many, 8), ("query_direct", self.few, 8), ("sample", self.few, 8),
            ("sample_plane", plane, 8), ("sample_lod", self.few, 8), ("sample_plane_lod", plane, 8),
            ("velocity", self.few, 8), ("kinematics", self.few, 12), ("raycast", self.rays, 16),
            ("sample_foam", self.few, 8), ("sample_plane_foam", plane, 8))}

    def calls(self, p):
        s, o, few = self.sampler, self.o, self.few
        return super().calls(p) + [
            lambda: s.query(self.in_many, self.many, 8, 0.0, o["query_atlas"]),
            lambda: s.query(self.in_xz, few, 8, 0.0, o["query_direct"]),
            lambda: s.sample(self.in_xz, few, o["sample"]),
            lambda: s.sample_plane(CAMERA, self.res, o["sample_plane"]),
            lambda: s.sample_lod(self.in_xzf, few, o["sample_lod"]),
            lambda: s.sample_plane_lod(CAMERA, self.res, o["sample_plane_lod"]),
            lambda: s.velocity(self.in_xz, few, o["velocity"]),
            lambda: s.kinematics(self.in_xyz, few, 8, 0.0, o["kinematics"]),
            lambda: s.raycast(self.in_rays, self.rays, o["raycast"]),
            lambda: s.sample_foam_device(self.in_xz, few, o["sample_foam"]),
            lambda: s.sample_plane_foam_device(CAMERA, self.res, o["sample_plane_foam"])]

    def products(self):
        return super().products() + list(self.outs)


@gpu
def test_point_consumers(ocean, stall):
    from test_item_loops import query_uses_atlas

    assert query_uses_atlas(3, 64, 70000, 8) and not query_uses_atlas(3, 64, 3000, 8)
    check(ocean, stall, [Points], label="Points")


# ---- d. the stateful chain -----------------------------------------------------------------------------
class Chain(Seq):
    """Three steps with no host wait: frame -> advance_foam -> spray.emit (device count) -> particles.step (landed
    list and its device count) -> foam_deposit from that list -> render_layers with the pool's records and device
    count (40 x 24) -> render; hulls.loads with poses produced on the stream. The pass begins with reset_foam and
    particles.clear: the foam and the pool are state that the sentinels overwrite."""

    W, H, STEPS = 40, 24, 3

    def __init__(self, ocean, stream):
        from oceansimulation_amd.surface import (HullSet, SprayEmitter, SprayParticles, SurfaceSampler,
                                                 camera_layers_scratch_bytes)
        from test_hulls import _random_points, _random_poses

        super().__init__(ocean, stream)
        self.fft = ocean.FFTCalculator(64, stream=stream)
        self.gen = g = ocean.Generator(self.fft, 3)
        for c, plane in enumerate(PLANES):
            ocean.apply_settings(g.GetOceanSettings(c), planeSize=plane)
            ocean.apply_foam_settings(g.GetFoamSettings(c), **FOAM)
        self.sampler = SurfaceSampler([(g, c) for c in range(3)])
        self.emitter = SprayEmitter(self.fft)
        self.capacity, self.emit_capacity = 4500, 3 * 64 * 64
        self.pool = SprayParticles(self.fft, self.capacity)
        rng = np.random.default_rng(9)
        points = _random_points(rng, 70)
        self.bodies = 40
        self.hulls = HullSet(self.fft, points, np.tile(np.array([[0, 70]], np.int32), (self.bodies, 1)))
        self.poses = self.input(_random_poses(rng, self.bodies))
        self.emitted = self.output("emitted", self.emit_capacity * 32, "some")
        self.impacts = self.output("impacts", self.capacity * 32, "some")
        self.loads = self.output("loads", self.bodies * 32)
        self.point_rows = self.output("hull_points", self.hulls.instance_points * 32)
        px = self.W * self.H
        self.scratch = self.output("layers_scratch", camera_layers_scratch_bytes(self.W, self.H), None)
        self.images = {name: self.output(name, px * size, mode) for name, size, mode in (
            ("layers_image", 16, "rows"), ("layers_aux", 16, "rows"), ("layers_aux2", 16, "some"),
            ("layers_image8", 4, "some"), ("image", 16, "rows"), ("aux", 16, "rows"), ("image8", 4, "some"))}

    def calls(self, p):
        from oceansimulation_amd.surface import default_camera_layers, default_march, default_shading
        from test_camera import _cam_a

        o, g, s, im = self.ocean, self.gen, self.sampler, self.images
        fly = o.default_particle_settings(lift=100.0, lifetime=0.6)
        spray = dict(threshold=1.0, rate=64.0, seed=12345)
        cam, shading, march = _cam_a(), default_shading(), default_march()
        layers = default_camera_layers(foam_lo=0.1, foam_hi=0.4, foam_opacity=0.8, spray_radius=0.2, spray_max_half=3,
                                       spray_opacity=0.3)
        out = []
        if p == 0:  # the particles read the rates of the frame; the renders read the bounds
            out += [lambda: g.CalculateOcean(1.0, True), lambda: g.advance_foam(DT), g.calculate_rates, g.build_bounds,
                    lambda: self.emitter.emit(s, spray, DT, 6, self.emitted, self.emit_capacity),
                    lambda: self.pool.step(s, fly, DT, emitter=self.emitter, emit_records=self.emitted,
                                           landed=self.impacts, landed_capacity=self.capacity),
                    lambda: s.deposit_foam(self.impacts, self.capacity, dict(amount=0.5, per_speed=0.05),
                                           self.pool.counts_device() + 4 * 8)]
        out += [g.reset_foam, self.pool.clear]
        for k in range(self.STEPS):
            step = 7 + 3 * p + k
            out += [lambda: g.CalculateOcean(DT), lambda: g.advance_foam(DT), g.calculate_rates, g.build_bounds,
                    lambda step=step: self.emitter.emit(s, spray, DT, step, self.emitted, self.emit_capacity),
                    lambda: self.pool.step(s, fly, DT, emitter=self.emitter, emit_records=self.emitted,
                                           landed=self.impacts, landed_capacity=self.capacity),
                    lambda: s.deposit_foam(self.impacts, self.capacity, dict(amount=0.5, per_speed=0.05),
                                           self.pool.counts_device() + 4 * 8),
                    lambda: s.render_layers(cam, shading, march, layers, self.W, self.H, im["layers_image"],
                                            im["layers_aux"], im["layers_aux2"], im["layers_image8"], particles=self.pool,
                                            scratch_ptr=self.scratch),
                    lambda: s.render(cam, shading, march, self.W, self.H, im["image"], im["aux"], im["image8"])]
        return out + [lambda: self.hulls.loads(s, self.poses, self.loads, self.point_rows, 9810.0, 8, 0.0, True)]

    def products(self):
        out = self.map_products(self.gen) + [(n, ptr, nb, m) for n, ptr, nb, m in self.outs if m is not None]
        out += [(f"foam{c}", self.gen.GetFoamMap(c), 64 * 64 * 4, "words") for c in range(3)]
        out += [("pool_counts", self.pool.counts_device(), 8 * 8, "some"),
                ("spray_counts", self.emitter.counts_device(), 18 * 8, "some"),
                ("deposit_counts", self.sampler.deposit_counts_device(), 50 * 8, "some")]
        return out

    def late(self):
        counts = self.pool.counts()
        assert counts[0] > 0 and counts[4] > 0, counts  # particles alive and landed: the chain carried records
        return {"pool_counts_host": counts, "pool_records": self.pool.records_host(np.uint32),
                "spray_counts_host": self.emitter.counts(), "deposit_counts_host": self.sampler.deposit_counts(),
                "foam_counts_host": np.stack([self.gen.GetFoamCounts(c) for c in range(3)])}

    def close(self):
        super().close()
        for h in (self.hulls, self.pool, self.emitter, self.gen, self.fft):
            h.close()


@gpu
def test_stateful_chain(ocean, stall):
    check(ocean, stall, [Chain], label="Chain")


# ---- e. calls with a stream argument of their own or a caller's image ----------------------------------------
class OwnStream(Seq):
    """ocean_fft_encode_ifft and _batch on images written on the stream (N = 256); ocean_camera_rays and
    ocean_debug_hash given the non-blocking stream."""

    def __init__(self, ocean, stream):
        super().__init__(ocean, stream)
        n = 256
        self.fft = ocean.FFTCalculator(n, stream=stream)
        rng = np.random.default_rng(2)
        self.images = rng.standard_normal((4, n, n, 4)).astype(np.float32)
        self.one = self.input(self.images[0])
        self.three = self.input(self.images[1:])
        self.count = 5000
        self.xy = self.input(rng.integers(0, 2 ** 32, (self.count, 2), dtype=np.uint32))
        self.raw = self.output("hash_raw", self.count * 4, None)
        self.uv = self.output("hash_uv", self.count * 8, None)
        self.rays = self.output("camera_rays", 40 * 24 * 32)

    def calls(self, p):
        from oceansimulation_amd import capi
        from oceansimulation_amd.waves import debug_hash
        from test_camera import _cam_a

        cam = _cam_a()
        L = capi.lib()

        def rays():
            capi.check(L.ocean_camera_rays(ctypes.byref(cam), 40, 24, ctypes.c_void_p(self.rays),
                                           ctypes.c_void_p(self.stream or 0)), "ocean_camera_rays")

        return [lambda: self.fft.EncodeIFFT(self.one), lambda: self.fft.encode_ifft_batch(self.three, 3), rays,
                lambda: debug_hash(self.xy, self.count, self.raw, self.uv, self.stream)]

    def products(self):
        n = 256
        # the transforms run in place: the "outputs" are the inputs the stream wrote
        return [(n_, p_, b_, "some" if m_ is None else m_) for n_, p_, b_, m_ in self.outs] + [
            ("ifft", self.one, n * n * 16, "rows"), ("ifft_batch", self.three, 3 * n * n * 16, "rows")]

    def close(self):
        super().close()
        self.fft.close()


@gpu
def test_own_stream_arguments(ocean, stall):
    check(ocean, stall, [OwnStream], label="OwnStream")


# ---- f. two plans on two non-blocking streams ---------------------------------------------------------------
class PointsB(Points):
    """A second scene on a plan of its own: other planes and other points."""

    planes, seed = (7.0, 29.0, 83.0), 6


@gpu
def test_two_plans_on_two_streams(ocean, stall):
    """The sequences of (b) and (c) of two scenes interleaved call by call, each behind a stall of its own length:
    each equals its own null-stream run, so the plan-owned scratch (atlas, work image) and the process-wide
    caches of launch_common.h do not couple plans."""
    check(ocean, stall, [Points, PointsB], stall_bytes=[STALL_BYTES, STALL_BYTES * 3 // 4], label="two plans")


# ---- the harness itself --------------------------------------------------------------------------------
@gpu
def test_null_stream_does_not_rescue_a_non_blocking_stream(ocean, stall):
    """With only the null stream and the caller's stream alive: after the enqueue and before the synchronise, a
    small hipMemcpy D2H of one output on the null stream returns the 0xFF sentinel, so a launch that escaped to the
    null stream would not have waited for the stream's work either."""
    from oceansimulation_amd import hip

    s = hip.stream_create(hip.STREAM_NON_BLOCKING)
    seq = None
    try:
        assert hip.stream_flags(s) & hip.STREAM_NON_BLOCKING
        seq = Frames64(ocean, s)
        run_pass([seq], 0, stall)
        ptr = seq.gen.GetJacobianMap(2)
        snaps, pending, _, seen = run_pass([seq], 1, stall, [STALL_BYTES], probe=lambda: hip.to_host(ptr, (64,), np.uint32))
        assert pending == [True]
        assert (seen == 0xFFFFFFFF).all(), seen
        _no_sentinel(snaps[0], "after the synchronise")
    finally:
        if seq is not None:
            seq.close()
        hip.synchronize()
        hip.stream_destroy(s)
