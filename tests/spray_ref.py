"""Spray emitters (include/oceanfft.h, "Spray emitters ...") restated in numpy with float32 arrays throughout, so
every operation rounds as the kernels' unfused fp32 does.

    predicate   d = threshold - J;  p = min((max(d, 0) * rate) * dt, 1)
                u = hash2(hash2(x, y).n ^ seed, step).u0 (numpy_ref.hash2: the denominator float(0x7FFFFFFF) is
                float32(2147483648.0));  emits = d > 0 and (p >= 1 or u < p)
    emit        the emitting texels of every pair in (pair, y * N + x) order: ids (pair << 28 | texel), d, the base
                points ((x + 0.5) * cell + tile * L with cell = L / N) and the int64[18] counts for a capacity
    records     the (written, 8) rows from emit's lists and the rows of a velocity (or vertex-stage) restatement
"""
import numpy as np

import numpy_ref as R

F = np.float32
COUNTS = 18


def predicate(jac, threshold, rate, seed, dt, step):
    """(emits, d, p) of one pair's (n, n) Jacobian map; x is the column, y the row."""
    jac = np.asarray(jac, F)
    n = jac.shape[0]
    y, x = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), indexing="ij")
    d = F(threshold) - jac
    p = np.minimum((np.maximum(d, F(0.0)) * F(rate)) * F(dt), F(1.0))
    first = R.hash2(x, y)[2]
    u = R.hash2(first ^ np.uint32(seed), np.full_like(first, np.uint32(step)))[0]
    emits = (d > 0) & ((p >= F(1.0)) | (u < p))
    return emits, d, p


def emit(jacs, planes, settings, dt, step, capacity=None, tiles=None):
    """jacs: one (n, n) map per pair; planes: their planeSize; settings: (threshold, rate, seed) per pair.
    Returns (ids uint32 (found,), d float32 (found,), base points float32 (found, 2), counts int64 (18,));
    capacity None: room for all."""
    ids, ds, bases = [], [], []
    counts = np.zeros(COUNTS, np.int64)
    for i, (jac, plane, (threshold, rate, seed)) in enumerate(zip(jacs, planes, settings)):
        n = jac.shape[0]
        if rate == 0:
            continue
        emits, d, _ = predicate(jac, threshold, rate, seed, dt, step)
        texel = np.flatnonzero(emits.ravel()).astype(np.uint32)
        x, y = texel % np.uint32(n), texel // np.uint32(n)
        cell = F(plane) / F(n)
        tx, tz = (0, 0) if tiles is None else tiles[i]
        bx = (x.astype(F) + F(0.5)) * cell + F(tx) * F(plane)
        bz = (y.astype(F) + F(0.5)) * cell + F(tz) * F(plane)
        ids.append((np.uint32(i) << np.uint32(28)) | texel)
        ds.append(d.ravel()[texel])
        bases.append(np.stack([bx, bz], -1).astype(F))
        counts[2 + i] = texel.size
    ids = np.concatenate(ids) if ids else np.zeros(0, np.uint32)
    ds = np.concatenate(ds) if ds else np.zeros(0, F)
    bases = np.concatenate(bases) if bases else np.zeros((0, 2), F)
    counts[1] = ids.size
    counts[0] = ids.size if capacity is None else min(ids.size, capacity)
    return ids, ds, bases, counts


def records(ids, ds, rows, written=None):
    """rows: (found, 8) float32 with slots 0-2 and 4-6 set (rates_ref.surface_velocity's, or a vertex stage's with
    zeros) -> the records: slot 3 = d, slot 7 = the id's bits."""
    out = np.array(rows, F, copy=True)
    out[:, 3] = ds
    out.view(np.uint32)[:, 7] = ids
    return out if written is None else out[:written]
