"""ocean_surface_query's contract (include/oceanfft.h) restated in numpy float32 on top of the oracle's
forward map: oracle.surface_points is ocean_surface_sample bit for bit, so no sampler is restated here.

    p = q
    repeat at most `iterations` times:
        r = q - V(p).xz
        if max(|r.x|, |r.z|) <= tolerance: stop
        p = p + r
    V = V(p)
    out = (p.x, V.y, p.z, V.jacobian, V.normal, max(|q.x - V.x|, |q.z - V.z|))
"""
import numpy as np


def surface_query(oracle, cascades, q, iterations, tolerance, with_used=False):
    """cascades: [(height, disp, jac, planeSize, displacement)] as oracle.surface_points takes them;
    q: (P, 2) world positions. Returns (P, 8) float32, and with with_used the iteration steps each
    point took."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 2)
    tol = np.float32(tolerance)
    p = q.copy()
    V = oracle.surface_points(cascades, p)
    active = np.ones(q.shape[0], bool)
    used = np.zeros(q.shape[0], np.int32)
    for _ in range(int(iterations)):
        r = (q - V[:, [0, 2]]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            active &= ~(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= tol)
        if not active.any():
            break
        p[active] = (p[active] + r[active]).astype(np.float32)
        V[active] = oracle.surface_points(cascades, np.ascontiguousarray(p[active]))
        used[active] += 1
    out = V.copy()
    out[:, 0] = p[:, 0]
    out[:, 2] = p[:, 1]
    out[:, 7] = np.maximum(np.abs(q[:, 0] - V[:, 0]), np.abs(q[:, 1] - V[:, 2]))
    return (out, used) if with_used else out
