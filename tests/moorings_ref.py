"""ocean_moorings_step's contract (include/oceanfft.h, "Mooring lines") restated in numpy float32 (TEST
INFRASTRUCTURE), on kinematics_ref.water_kinematics (the water at a node) and hull_loads_ref's pose layout.
Every operation is a float32 array operation over all nodes (or lines) at once, in the order the header writes
it, so it rounds as the kernel's unfused fp32: sqrt and division are correctly rounded on both sides.

    line(...)                       one row of ocean_moorings_create's lines
    constants(lines, attach)        the per-line constants the host builds, in float32
    fairleads(lines, attach, poses) d, P, vp per line
    reset(lines, attach, poses)     ocean_moorings_reset -> nodes (total, 8)
    mooring_step(lines, attach, nodes, poses, bodies, dt, substeps, ..., water_fn, dtype)
                                    one call -> (nodes, line_out, wrench_ext)
    water(oracle, cascades, layers, depths, iterations, tolerance)   the water_fn of settings.water == 1

dtype=float64 evaluates the same recurrence in double precision on the same float32 inputs (the yardstick of the
closed-form tests); only still water is restated in it.
"""
import numpy as np

import kinematics_ref as K

F = np.float32
GRAVITY = (0.0, -9.8, 0.0)
DEFAULTS = dict(dt=1.0 / 60.0, substeps=8, gravity=GRAVITY, rho_g=9810.0, bed_y=-100.0, bed_k=1e5, bed_c=1e3)


def line(anchor, fairlead, length, ea, ca=0.0, mass_per_m=1.0, volume_per_m=0.0, drag_lin=0.0, drag_quad=0.0):
    out = np.zeros(16, F)
    out[0:3], out[3:6] = anchor, fairlead
    out[6:13] = length, ea, ca, mass_per_m, volume_per_m, drag_lin, drag_quad
    return out


def constants(lines, attach):
    """dict of float32 arrays per line: l0 and the lumps mn, vn, dl, dq."""
    lines = np.ascontiguousarray(lines, F).reshape(-1, 16)
    nodes = np.ascontiguousarray(attach, np.int32).reshape(-1, 2)[:, 1]
    l0 = lines[:, 6] / (nodes - 1).astype(F)
    c = dict(l0=l0, ea=lines[:, 7], ca=lines[:, 8], mn=lines[:, 9] * l0, vn=lines[:, 10] * l0, dl=lines[:, 11] * l0,
             dq=lines[:, 12] * l0)
    assert all(v.dtype == F for v in c.values())
    return c


def fairleads(lines, attach, poses, dtype=F):
    """(d, P, vp), each (lines, 3): ocean_hulls_loads' expressions; body -1: d = 0, P = Lf, vp = 0."""
    lines = np.ascontiguousarray(lines, F).reshape(-1, 16).astype(dtype)
    body = np.ascontiguousarray(attach, np.int32).reshape(-1, 2)[:, 0]
    Lf = lines[:, 3:6]
    d, P, vp = np.zeros_like(Lf), Lf.copy(), np.zeros_like(Lf)
    on = body >= 0
    if on.any():
        Q = np.ascontiguousarray(poses, F).reshape(-1, 20).astype(dtype)[body[on]]
        lx, ly, lz = Lf[on, 0], Lf[on, 1], Lf[on, 2]
        dd = [(Q[:, 3 * r] * lx + Q[:, 3 * r + 1] * ly) + Q[:, 3 * r + 2] * lz for r in range(3)]
        v, w = Q[:, 12:15], Q[:, 15:18]
        vv = [v[:, 0] + (w[:, 1] * dd[2] - w[:, 2] * dd[1]),
              v[:, 1] + (w[:, 2] * dd[0] - w[:, 0] * dd[2]),
              v[:, 2] + (w[:, 0] * dd[1] - w[:, 1] * dd[0])]
        d[on] = np.stack(dd, -1)
        P[on] = np.stack([Q[:, 9 + r] + dd[r] for r in range(3)], -1)
        vp[on] = np.stack(vv, -1)
    assert d.dtype == dtype and P.dtype == dtype and vp.dtype == dtype
    return d, P, vp


def _layout(attach):
    nodes = np.ascontiguousarray(attach, np.int32).reshape(-1, 2)[:, 1]
    offs = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
    ln = np.repeat(np.arange(nodes.shape[0]), nodes)       # the node's line
    i = np.arange(offs[-1]) - offs[ln]                      # its index in the line
    return nodes, offs, ln, i


def reset(lines, attach, poses=None):
    lines = np.ascontiguousarray(lines, F).reshape(-1, 16)
    nodes, _, ln, i = _layout(attach)
    _, P, _ = fairleads(lines, attach, poses)
    A = lines[:, 0:3]
    t = i.astype(F) / (nodes[ln] - 1).astype(F)
    out = np.zeros((ln.shape[0], 8), F)
    out[:, 0:3] = A[ln] + t[:, None] * (P[ln] - A[ln])
    return out


def still_water(xyz):
    """water_fn of settings.water == 0: u = 0, wet = (0 - y) > 0."""
    y = xyz[:, 1]
    return np.zeros_like(xyz), (y.dtype.type(0.0) - y) > 0


def water(oracle, cascades, layers, depths, iterations=4, tolerance=0.0):
    """water_fn of settings.water == 1 over kinematics_ref.water_kinematics: slots 4..6 and 11."""
    def fn(xyz):
        out = K.water_kinematics(oracle, cascades, layers, depths, xyz, iterations, tolerance)
        return out[:, 4:7], out[:, 11] != 0
    return fn


def mooring_step(lines, attach, nodes, poses, bodies, dt=DEFAULTS["dt"], substeps=DEFAULTS["substeps"],
                 gravity=GRAVITY, rho_g=DEFAULTS["rho_g"], bed_y=DEFAULTS["bed_y"], bed_k=DEFAULTS["bed_k"],
                 bed_c=DEFAULTS["bed_c"], water_fn=still_water, dtype=F):
    """One ocean_moorings_step call: (nodes (total, 8), line_out (lines, 8), wrench_ext (bodies, 8))."""
    T_ = dtype
    lines = np.ascontiguousarray(lines, F).reshape(-1, 16)
    att = np.ascontiguousarray(attach, np.int32).reshape(-1, 2)
    n_nodes, offs, ln, i = _layout(att)
    total = ln.shape[0]
    c = {k: v.astype(T_) for k, v in constants(lines, att).items()}
    d, P, vp = fairleads(lines, att, poses, T_)
    A = lines[:, 0:3].astype(T_)
    h = T_(F(dt) / F(substeps))  # the float32 quotient in either type
    g = [T_(F(x)) for x in gravity]
    rho_g, bed_y = T_(F(rho_g)), T_(F(bed_y))
    kb, cb = T_(F(bed_k)) * c["l0"], T_(F(bed_c)) * c["l0"]
    zero = T_(0.0)

    first, last = i == 0, i == n_nodes[ln] - 1
    interior, segment = ~first & ~last, ~last
    N = np.ascontiguousarray(nodes, T_).reshape(total, 8)  # float64 keeps its state between calls
    x, v = N[:, 0:3].copy(), N[:, 4:7].copy()
    x[first], v[first] = A[ln[first]], zero
    x[last], v[last] = P[ln[last]], vp[ln[last]]
    nxt, prv = np.minimum(np.arange(total) + 1, total - 1), np.maximum(np.arange(total) - 1, 0)
    l0, ea, ca, mn, vn, dl, dq = (c[k][ln] for k in ("l0", "ea", "ca", "mn", "vn", "dl", "dq"))
    kbn, cbn = kb[ln], cb[ln]
    fair = offs[1:] - 2  # the node that keeps the fairlead segment
    total_f = np.zeros((lines.shape[0], 3), T_)
    T = np.zeros(total, T_)
    wet = bed = np.zeros(total, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(substeps)):
            dv = x[nxt] - x
            ln_ = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
            e = np.where((ln_ > 0)[:, None], dv / ln_[:, None], zero).astype(T_)
            strain = (ln_ - l0) / l0
            dw = v[nxt] - v
            rate = ((dw[:, 0] * e[:, 0] + dw[:, 1] * e[:, 1]) + dw[:, 2] * e[:, 2]) / l0
            t = ea * strain + ca * rate
            T = np.where(segment & (t > 0), t, zero).astype(T_)  # NaN -> 0
            e[~segment] = zero
            S = T[:, None] * e
            total_f = total_f + (-S[fair])
            u, w_ = water_fn(x)
            u, wet = u.astype(T_), np.asarray(w_, bool) & interior
            rel = u - v
            m = np.sqrt((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2])
            k = np.where(wet, dl + dq * m, zero).astype(T_)
            Fo = [((S[:, a] - S[prv, a]) + k * rel[:, a]) + mn * g[a] for a in range(3)]
            Fo[1] = np.where(wet, Fo[1] + rho_g * vn, Fo[1])
            pen = bed_y - x[:, 1]
            bed = (pen > 0) & interior
            Fo[1] = np.where(bed, Fo[1] + kbn * pen, Fo[1])
            Fo = [np.where(bed, Fo[a] - cbn * v[:, a], Fo[a]) for a in range(3)]
            v1 = np.stack([v[:, a] + h * (Fo[a] / mn) for a in range(3)], -1)
            x1 = x + h * v1
            assert v1.dtype == T_ and x1.dtype == T_ and T.dtype == T_ and S.dtype == T_
            v = np.where(interior[:, None], v1, v)
            x = np.where(interior[:, None], x1, x)
    out = np.zeros((total, 8), T_)
    out[:, 0:3], out[:, 3], out[:, 4:7] = x, T, v
    out[:, 7] = wet.astype(T_) + T_(2.0) * bed.astype(T_)
    Fm = total_f / T_(F(substeps))
    line_out = np.zeros((lines.shape[0], 8), T_)
    line_out[:, 0:3], line_out[:, 3], line_out[:, 4] = Fm, T[fair], T[offs[:-1]]
    line_out[:, 5] = np.maximum.reduceat(T, offs[:-1])
    line_out[:, 6] = np.add.reduceat(bed.astype(np.int64), offs[:-1]).astype(T_)
    line_out[:, 7] = np.add.reduceat(wet.astype(np.int64), offs[:-1]).astype(T_)
    wrench = np.zeros((int(bodies), 8), T_)
    for li in range(lines.shape[0]):  # ascending line index, from +0.0
        b = att[li, 0]
        if b < 0:
            continue
        f, dd = Fm[li], d[li]
        wrench[b, 0:3] = wrench[b, 0:3] + f
        wrench[b, 4] = wrench[b, 4] + (dd[1] * f[2] - dd[2] * f[1])
        wrench[b, 5] = wrench[b, 5] + (dd[2] * f[0] - dd[0] * f[2])
        wrench[b, 6] = wrench[b, 6] + (dd[0] * f[1] - dd[1] * f[0])
        wrench[b, 3] = wrench[b, 3] + T_(1.0)
    return out, line_out, wrench
