"""ocean_hulls_loads' contract (include/oceanfft.h, "Hull sets") restated in numpy float32 (TEST
INFRASTRUCTURE), on top of surface_query_ref.surface_query (the water above a world position) and
rates_ref.surface_velocity (the water particle's velocity). Every operation is a float32 array operation,
so it rounds as the kernel's unfused fp32; fold64 and tree_sum are the contract's summation order, literally:

    fold64(a): pad a (len <= 64) with +0.0f to 64; for h in 32,16,8,4,2,1: a = a[:h] + a[h:]; return a[0]
    sum(a):    len <= 64 -> fold64(a); else sum([fold64(a[j:j+64]) for j in 0,64,128,...])
"""
import numpy as np

import rates_ref
from surface_query_ref import surface_query

F = np.float32
U = 2.0 ** -24  # unit roundoff of fp32


def fold64(a):
    """a: (len <= 64,) or (len <= 64, C) float32 -> the fold of axis 0."""
    a = np.asarray(a, F)
    assert 1 <= a.shape[0] <= 64
    pad = np.zeros((64,) + a.shape[1:], F)  # +0.0f
    pad[:a.shape[0]] = a
    a = pad
    for h in (32, 16, 8, 4, 2, 1):
        a = (a[:h] + a[h:]).astype(F)
    return a[0]


def tree_sum(a):
    a = np.asarray(a, F)
    if a.shape[0] <= 64:
        return fold64(a)
    return tree_sum(np.stack([fold64(a[j:j + 64]) for j in range(0, a.shape[0], 64)]))


def box_hull(nx=4, ny=4, nz=4, size=(2.0, 1.0, 4.0), drag_lin=40.0, drag_quad=15.0):
    """nx * ny * nz points at the cell centres of a box, x fastest: (lx, ly, lz, cell volume, half the cell's
    height, drag_lin, drag_quad, 0)."""
    cx, cy, cz = size[0] / nx, size[1] / ny, size[2] / nz
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.zeros((nx * ny * nz, 8), F)
    pts[:, 0] = ((i.ravel() + 0.5) * cx - size[0] / 2)
    pts[:, 1] = ((j.ravel() + 0.5) * cy - size[1] / 2)
    pts[:, 2] = ((k.ravel() + 0.5) * cz - size[2] / 2)
    pts[:, 3] = cx * cy * cz
    pts[:, 4] = cy / 2
    pts[:, 5] = drag_lin
    pts[:, 6] = drag_quad
    return pts


def pose(R=None, c=(0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0), w=(0.0, 0.0, 0.0)):
    """One row of poses: R[9] row-major body->world, c, v, w, 0, 0."""
    out = np.zeros(20, F)
    out[:9] = np.eye(3, dtype=F).ravel() if R is None else np.asarray(R, F).ravel()
    out[9:12], out[12:15], out[15:18] = c, v, w
    return out


def hull_loads(oracle, cascades, rates, points, ranges, poses, rho_g, iterations, tolerance, water_velocity):
    """cascades: [(height, disp, jac, planeSize, displacement)], rates: [(height_rate, disp_rate)] or None
    when not water_velocity. Returns (loads (bodies, 8), point_out (instance points, 8), info) with info =
    dict(x: world points, u: water velocity, s: submerged fraction, used: query steps, a: the terms a_i)."""
    points = np.ascontiguousarray(points, F).reshape(-1, 8)
    ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 2)
    poses = np.ascontiguousarray(poses, F).reshape(ranges.shape[0], 20)
    body = np.repeat(np.arange(ranges.shape[0]), ranges[:, 1])
    offs = np.concatenate([[0], np.cumsum(ranges[:, 1])])
    idx = np.concatenate([np.arange(f, f + n) for f, n in ranges])
    L, P = points[idx], poses[body]
    lx, ly, lz = L[:, 0], L[:, 1], L[:, 2]
    d = [(P[:, 3 * r] * lx + P[:, 3 * r + 1] * ly) + P[:, 3 * r + 2] * lz for r in range(3)]
    x = [P[:, 9 + r] + d[r] for r in range(3)]
    q = np.stack([x[0], x[2]], -1).astype(F)
    Q, used = surface_query(oracle, cascades, q, iterations, tolerance, with_used=True)
    eta, res = Q[:, 1], Q[:, 7]
    base = np.ascontiguousarray(Q[:, [0, 2]])
    with np.errstate(invalid="ignore"):
        t = (eta - x[1]) / (L[:, 4] + L[:, 4]) + F(0.5)
        s = np.where(t > 0, np.minimum(t, F(1.0)), F(0.0)).astype(F)  # NaN -> 0
    if water_velocity:
        u = rates_ref.surface_velocity(cascades, rates, base)[:, 4:7]
    else:
        u = np.zeros((q.shape[0], 3), F)
    v, w = P[:, 12:15], P[:, 15:18]
    vp = [v[:, 0] + (w[:, 1] * d[2] - w[:, 2] * d[1]),
          v[:, 1] + (w[:, 2] * d[0] - w[:, 0] * d[2]),
          v[:, 2] + (w[:, 0] * d[1] - w[:, 1] * d[0])]
    rel = [u[:, r] - vp[r] for r in range(3)]
    m = np.sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2])
    k = s * (L[:, 5] + L[:, 6] * m)
    vs = L[:, 3] * s
    Fx, Fy, Fz = k * rel[0], F(rho_g) * vs + k * rel[1], k * rel[2]
    Tx, Ty, Tz = d[1] * Fz - d[2] * Fy, d[2] * Fx - d[0] * Fz, d[0] * Fy - d[1] * Fx
    a = np.stack([Fx, Fy, Fz, vs, Tx, Ty, Tz, (s > 0).astype(F)], -1).astype(F)
    assert all(z.dtype == F for z in (t, m, k, Fx, Fy, Tz))
    point_out = np.stack([base[:, 0], eta, base[:, 1], res, Fx, Fy, Fz, s], -1).astype(F)
    loads = np.stack([tree_sum(a[offs[b]:offs[b + 1]]) for b in range(ranges.shape[0])])
    return loads, point_out, dict(x=np.stack(x, -1), u=u, s=s, used=used, a=a, offsets=offs)
