"""ocean_hulls_step's contract (include/oceanfft.h, "Hull dynamics") restated in numpy float32 (TEST
INFRASTRUCTURE) on hull_loads_ref.hull_loads. Every operation is a float32 array operation over the bodies,
in the order the header writes it, so it rounds as the kernel's unfused fp32: sqrt and division are correctly
rounded on both sides and nothing else is used.

    integrate(poses, loads, props, h, gravity, ext)   one substep from given loads
    hull_step(loads_fn, poses, props, dt, substeps, gravity, ext)   one call: h = dt / substeps in float32,
        per substep loads_fn(poses) -> (loads, point_out), then integrate
    water_loads(oracle, cascades, rates, points, ranges, ...)   the loads_fn over hull_loads_ref.hull_loads
"""
import numpy as np

import hull_loads_ref as H

F = np.float32
GRAVITY = (0.0, -9.8, 0.0)


def props(mass, inertia, lin_damp=0.0, ang_damp=0.0, kinematic=0.0):
    """One row of ocean_hulls_set_bodies' props."""
    return np.array([mass, inertia[0], inertia[1], inertia[2], lin_damp, ang_damp, kinematic, 0.0], F)


def box_inertia(mass, size):
    """Principal moments of a uniform box."""
    x, y, z = size
    return (mass * (y * y + z * z) / 12.0, mass * (x * x + z * z) / 12.0, mass * (x * x + y * y) / 12.0)


def integrate(poses, loads, props, h, gravity=GRAVITY, ext=None, dtype=F):
    """One substep of every body: (bodies, 20) poses -> the stepped poses, from loads (bodies, 8). dtype
    float64 evaluates the same recurrence in double precision (the yardstick of the closed-form tests)."""
    F = dtype  # noqa: N806 (every operation below is in this type)
    P = np.ascontiguousarray(poses, F).reshape(-1, 20)
    Lb = np.ascontiguousarray(loads, F).reshape(-1, 8)
    pr = np.ascontiguousarray(props, F).reshape(-1, 8)
    h = F(h)
    g = [F(np.float32(x)) for x in gravity]  # the float32 inputs in either type
    one, two, half = F(1.0), F(2.0), F(0.5)
    R = [[P[:, 3 * i + j] for j in range(3)] for i in range(3)]
    c, v, w = [P[:, 9 + k] for k in range(3)], [P[:, 12 + k] for k in range(3)], [P[:, 15 + k] for k in range(3)]
    Fo, T = [Lb[:, k] for k in range(3)], [Lb[:, 4 + k] for k in range(3)]
    if ext is not None:
        E = np.ascontiguousarray(ext, F).reshape(-1, 8)
        Fo = [Fo[k] + E[:, k] for k in range(3)]
        T = [T[k] + E[:, 4 + k] for k in range(3)]
    mass, I, lin, ang, kin = pr[:, 0], [pr[:, 1 + k] for k in range(3)], pr[:, 4], pr[:, 5], pr[:, 6] != 0
    with np.errstate(all="ignore"):
        kl, ka = one + h * lin, one + h * ang
        vd = [(v[k] + h * (Fo[k] / mass + g[k])) / kl for k in range(3)]
        wb = [(R[0][k] * w[0] + R[1][k] * w[1]) + R[2][k] * w[2] for k in range(3)]
        Tb = [(R[0][k] * T[0] + R[1][k] * T[1]) + R[2][k] * T[2] for k in range(3)]
        L = [I[k] * wb[k] for k in range(3)]
        G = [wb[1] * L[2] - wb[2] * L[1], wb[2] * L[0] - wb[0] * L[2], wb[0] * L[1] - wb[1] * L[0]]
        wn = [(wb[k] + h * ((Tb[k] - G[k]) / I[k])) / ka for k in range(3)]
        wd = [(R[k][0] * wn[0] + R[k][1] * wn[1]) + R[k][2] * wn[2] for k in range(3)]
        v1 = [np.where(kin, v[k], vd[k]) for k in range(3)]
        w1 = [np.where(kin, w[k], wd[k]) for k in range(3)]
        c1 = [c[k] + h * v1[k] for k in range(3)]
        hh = half * h
        a = [hh * w1[k] for k in range(3)]
        n = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        p, q = one - n, one + n
        xy, xz, yz = two * (a[0] * a[1]), two * (a[0] * a[2]), two * (a[1] * a[2])
        ux, uy, uz = two * a[0], two * a[1], two * a[2]
        Q = [[(p + two * (a[0] * a[0])) / q, (xy - uz) / q, (xz + uy) / q],
             [(xy + uz) / q, (p + two * (a[1] * a[1])) / q, (yz - ux) / q],
             [(xz - uy) / q, (yz + ux) / q, (p + two * (a[2] * a[2])) / q]]
        R1 = [[(Q[i][0] * R[0][j] + Q[i][1] * R[1][j]) + Q[i][2] * R[2][j] for j in range(3)] for i in range(3)]
        r0, r1 = R1[0], R1[1]
        l0 = np.sqrt((r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2])
        e0 = [r0[k] / l0 for k in range(3)]
        d = (e0[0] * r1[0] + e0[1] * r1[1]) + e0[2] * r1[2]
        u = [r1[k] - d * e0[k] for k in range(3)]
        l1 = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        e1 = [u[k] / l1 for k in range(3)]
        e2 = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
    cols = e0 + e1 + e2 + c1 + v1 + w1
    assert all(x.dtype == F for x in cols)
    out = np.zeros_like(P)  # slots 18 and 19: 0
    out[:, :18] = np.stack(cols, -1)
    return out


def hull_step(loads_fn, poses, props, dt, substeps, gravity=GRAVITY, ext=None, dtype=F):
    """One ocean_hulls_step call: (poses, loads, point_out), the last two of the last substep's start pose."""
    poses = np.ascontiguousarray(poses, dtype).reshape(-1, 20).copy()
    h = dtype(F(dt) / F(substeps))  # the float32 quotient in either type
    loads = pts = None
    for _ in range(int(substeps)):
        loads, pts = loads_fn(poses)
        poses = integrate(poses, loads, props, h, gravity, ext, dtype)
    return poses, loads, pts


def water_loads(oracle, cascades, rates, points, ranges, rho_g=9810.0, iterations=8, tolerance=0.0,
                water_velocity=False):
    """loads_fn of hull_step over hull_loads_ref.hull_loads on the given maps."""
    def fn(poses):
        loads, pts, _ = H.hull_loads(oracle, cascades, rates, points, ranges, poses, rho_g, iterations, tolerance,
                                     water_velocity)
        return loads, pts
    return fn


def dry_loads(poses):
    """loads_fn of bodies with no water under them: every load is +0."""
    return np.zeros((np.asarray(poses).reshape(-1, 20).shape[0], 8), F), None
