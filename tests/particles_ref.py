"""Spray particles (include/oceanfft.h, "Spray particles ...") restated in numpy with float32 arrays throughout, so
every operation rounds as the kernels' unfused fp32 does. The water height under a particle is
surface_query_ref.surface_query's slot 1 (the query's contract on the oracle's forward map), not a sampler of
its own.

    step    one ocean_particles_step on a list of (alive, 8) records: the next list (survivors in order, then the
            appended emitter records), every landed record in order, and the int64[8] counts
    launch  emitter records -> launched particles

Records travel as uint32 rows: slot 7 is a bit pattern (often a NaN as a float) and must not pass through
arithmetic.
"""
import numpy as np

import surface_query_ref as Q

F = np.float32
COUNTS = 8
DEFAULTS = dict(gravity=9.8, drag=0.5, wind=(0.0, 0.0, 0.0), lifetime=4.0, gain=1.0, lift=10.0, iterations=4,
                tolerance=1e-3)


def settings(**overrides):
    s = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def _rows(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.reshape(-1, 8).view(np.uint32).copy()


def launch(emit, s):
    """(E, 8) emitter records (px, py, pz, d, ux, uy, uz, id) -> launched particles as uint32 rows."""
    bits = _rows(emit)
    e = bits.view(F)
    out = bits.copy()
    o = out.view(F)
    gain, lift = F(s["gain"]), F(s["lift"])
    o[:, 3] = F(0.0)
    o[:, 4] = gain * e[:, 4]
    o[:, 5] = gain * e[:, 5] + lift * e[:, 3]
    o[:, 6] = gain * e[:, 6]
    return out


def step(oracle, cascades, records, s, dt, emit=None, capacity=None, landed_capacity=None):
    """records: (alive, 8) rows of 4-byte words; cascades as oracle.surface_points takes them; emit: the emitter's
    written records or None; capacity: the pool's (None: room for all); landed_capacity: None counts all as
    written. Returns (next list, landed records (all that were found), counts), the lists as uint32 rows."""
    bits = _rows(records)
    r = bits.view(F)
    dt = F(dt)
    alive = r.shape[0]
    drag, gravity = F(s["drag"]), F(s["gravity"])
    wind = [F(v) for v in s["wind"]]
    with np.errstate(invalid="ignore", over="ignore"):
        ax = drag * (wind[0] - r[:, 4])
        ay = drag * (wind[1] - r[:, 5]) - gravity
        az = drag * (wind[2] - r[:, 6])
        ux, uy, uz = r[:, 4] + ax * dt, r[:, 5] + ay * dt, r[:, 6] + az * dt
        px, py, pz = r[:, 0] + ux * dt, r[:, 1] + uy * dt, r[:, 2] + uz * dt
        age = r[:, 3] + dt
        w = np.zeros(0, F)
        if alive:
            w = Q.surface_query(oracle, cascades, np.stack([px, pz], -1), s["iterations"], s["tolerance"])[:, 1]
        landed = ~(py > w)
        expired = ~landed & ~(age < F(s["lifetime"]))
    survives = ~landed & ~expired
    moved = bits.copy()
    m = moved.view(F)
    for slot, v in enumerate((px, py, pz, age, ux, uy, uz)):
        m[:, slot] = v
    hit = moved[landed].copy()
    hit.view(F)[:, 1] = w[landed]
    nxt = moved[survives]
    counts = np.zeros(COUNTS, np.int64)
    n_surv, n_landed = int(survives.sum()), int(landed.sum())
    appended = emitted = 0
    if emit is not None:
        new = launch(emit, s)
        emitted = new.shape[0]
        appended = emitted if capacity is None else min(emitted, capacity - n_surv)
        nxt = np.concatenate([nxt, new[:appended]])
    counts[:] = (n_surv + appended, alive, n_surv, n_landed,
                 n_landed if landed_capacity is None else min(n_landed, landed_capacity), int(expired.sum()), appended,
                 emitted - appended)
    return nxt, hit, counts
