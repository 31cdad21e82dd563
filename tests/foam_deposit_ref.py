"""ocean_foam_deposit (include/oceanfft.h, "Foam deposit ...") restated in numpy: float32 arrays for every
floating-point operation, so each rounds as the kernels' unfused fp32 does, and uint64 for the units.

    taps     linear_repeat_taps (device/surface_sample.h) at (px / L, pz / L), operation by operation: the
             arithmetic of surface_lod_ref.bilinear, which reads a map through the same taps
    units    d = amount + per_speed * max(-uy, 0);  m = min(d * w, 1);  u = (uint64)(m * 2^24)
    deposit  A[o] += u with np.add.at;  F[t] = min(F[t] + (float)min(A[t], 2^24) * 2^-24, 1) where A[t] > 0
             counts = int64[50]: n, offered, then (taps with u > 0, texels touched, touched with F + add >= 1) per pair
"""
import numpy as np

F = np.float32
ONE = 1 << 24
COUNTS = 50
DEFAULTS = (0.05, 0.01)


def taps(n, px, pz, plane):
    """(offsets int64 (P, 4), weights float32 (P, 4)) in the order (i0, j0), (i1, j0), (i0, j1), (i1, j1)."""
    px, pz = np.asarray(px, F), np.asarray(pz, F)
    u, v = px / F(plane), pz / F(plane)
    s, t = u * F(n) - F(0.5), v * F(n) - F(0.5)
    fs, ft = np.floor(s), np.floor(t)
    a, b = s - fs, t - ft
    i0, j0 = fs.astype(np.int64) % n, ft.astype(np.int64) % n
    i1, j1 = (i0 + 1) % n, (j0 + 1) % n
    one = F(1.0)
    o = np.stack([j0 * n + i0, j0 * n + i1, j1 * n + i0, j1 * n + i1], -1)
    w = np.stack([(one - a) * (one - b), a * (one - b), (one - a) * b, a * b], -1)
    return o, w


def units(w, uy, amount, per_speed):
    """uint64 (P, 4)"""
    d = F(amount) + F(per_speed) * np.maximum(-np.asarray(uy, F), F(0.0))
    m = np.minimum(d[:, None] * w, F(1.0))
    return (m * F(16777216.0)).astype(np.uint64)  # truncation; m >= 0


def accumulate(n, plane, records, amount, per_speed):
    """One pair's accumulators: (A uint64 (n * n,), taps per texel int64 (n * n,)) of records (P, 8) 4-byte rows."""
    rec = np.ascontiguousarray(records).reshape(-1, 8).view(F)
    o, w = taps(n, rec[:, 0], rec[:, 2], plane)
    u = units(w, rec[:, 5], amount, per_speed)
    hit = u > 0
    acc = np.zeros(n * n, np.uint64)
    np.add.at(acc, o[hit], u[hit])
    return acc, np.bincount(o[hit], minlength=n * n).astype(np.int64)


def deposit(foams, planes, settings, records, offered=None):
    """foams: one (n, n) float32 map per pair; settings: (amount, per_speed) per pair; records (P, 8), all of them
    deposited. Returns (the maps after the call, counts int64[50]); offered: counts[1] (None: P)."""
    rec = np.ascontiguousarray(records).reshape(-1, 8)
    counts = np.zeros(COUNTS, np.int64)
    counts[0] = rec.shape[0]
    counts[1] = rec.shape[0] if offered is None else offered
    out = []
    for i, (fm, plane, (amount, per_speed)) in enumerate(zip(foams, planes, settings)):
        fm = np.ascontiguousarray(fm, F)
        n = fm.shape[0]
        if F(amount) == 0 and F(per_speed) == 0:
            out.append(fm.copy())
            continue
        acc, mult = accumulate(n, plane, rec, amount, per_speed)
        touched = acc > 0
        add = np.minimum(acc, np.uint64(ONE)).astype(F) * F(2.0 ** -24)
        total = fm.reshape(-1) + add
        out.append(np.where(touched, np.minimum(total, F(1.0)), fm.reshape(-1)).reshape(n, n))
        counts[2 + 3 * i] = mult.sum()
        counts[3 + 3 * i] = np.count_nonzero(touched)
        counts[4 + 3 * i] = np.count_nonzero(touched & (total >= F(1.0)))
    return out, counts
