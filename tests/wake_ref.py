"""The wake window's contract (include/oceanfft.h, "Wake windows") restated in numpy float32 / int64: the taps by
quadrature, the symbol, the stability bound, the splat through np.add.at on int64, the substep in the contract's
summation order, the shift and the sampler. Every float32 expression is evaluated in the order the header writes it,
one rounding per operation, so the device can be compared bit for bit."""
import numpy as np

F = np.float32
R = 6  # the operator's radius: 13 x 13 taps
UNITS = F(1048576.0)  # 2^20: the accumulators' units and the clamp
DEFAULTS = dict(dt=1.0 / 60.0, substeps=4, gravity=9.8, rho_g=9810.0, damp=0.05, edge_damp=8.0, border=16)


# ---- the taps ---------------------------------------------------------------------------------------
def taps_quadrature(sigma, nodes=400, angles=256):
    """T[a][b] = (1 / 2 pi) int_0^inf q^2 exp(-sigma q^2) J0(q r) dq, r = sqrt(a^2 + b^2), in float64:
    Gauss-Legendre in q on [0, 12 / sqrt(sigma)] (the integrand is below exp(-144) past it) and
    J0(x) = (1 / pi) int_0^pi cos(x sin t) dt by the midpoint rule, which converges geometrically for a periodic
    analytic integrand."""
    x, w = np.polynomial.legendre.leggauss(nodes)
    top = 12.0 / np.sqrt(sigma)
    q = 0.5 * top * (x + 1.0)
    w = 0.5 * top * w
    t = (np.arange(angles) + 0.5) * (np.pi / angles)
    out = np.zeros((R + 1, R + 1))
    for a in range(R + 1):
        for b in range(R + 1):
            r = np.sqrt(float(a * a + b * b))
            j0 = np.cos(np.outer(q * r, np.sin(t))).mean(axis=1)
            out[a, b] = np.sum(w * q * q * np.exp(-sigma * q * q) * j0) / (2.0 * np.pi)
    return out


def full_kernel(taps):
    """The 13 x 13 operator of the 7 x 7 taps, in the taps' dtype."""
    taps = np.asarray(taps).reshape(R + 1, R + 1)
    idx = np.abs(np.arange(-R, R + 1))
    return taps[np.ix_(idx, idx)]


def symbol_min(taps, grid=257):
    """The smallest value of the double cosine sum of the float taps over grid^2 points of [-pi, pi]^2."""
    k = -np.pi + 2.0 * np.pi * np.arange(grid) / (grid - 1)
    t = np.asarray(taps, np.float64).reshape(R + 1, R + 1)
    wgt = np.where(np.arange(R + 1) == 0, 1.0, 2.0)
    c = np.cos(np.outer(k, np.arange(R + 1))) * wgt  # [grid][a]
    return float((c @ t @ c.T).min())


def symbol(taps, kx, ky=0.0):
    t = np.asarray(taps, np.float64).reshape(R + 1, R + 1)
    wgt = np.where(np.arange(R + 1) == 0, 1.0, 2.0)
    return float((np.cos(kx * np.arange(R + 1)) * wgt) @ t @ (np.cos(ky * np.arange(R + 1)) * wgt))


def max_substep(taps, dx, gravity):
    """2 sqrt(dx / (gravity sum|T|)) over all 169 float taps, in float64 from the float arguments."""
    total = float(np.abs(full_kernel(np.asarray(taps, F)).astype(np.float64)).sum())
    return 2.0 * np.sqrt(float(F(dx)) / (float(F(gravity)) * total))


# ---- the window -------------------------------------------------------------------------------------
class Window:
    """h, h_prev and the integer offsets of one window; `taps` are the library's float taps (49)."""

    def __init__(self, size, dx, origin_x, origin_z, taps):
        self.m = int(size)
        self.dx = F(dx)
        self.origin = (F(origin_x), F(origin_z))
        self.off = [0, 0]
        self.taps = np.asarray(taps, F).reshape(R + 1, R + 1)
        self.h = np.zeros((self.m, self.m), F)  # [j][i]
        self.h_prev = np.zeros((self.m, self.m), F)
        self.hs = F(0.0)  # the last call's substep; 0: no step yet

    def ox(self):
        return F(self.origin[0] + F(F(self.off[0]) * self.dx))

    def oz(self):
        return F(self.origin[1] + F(F(self.off[1]) * self.dx))

    def reset(self):
        self.h[:] = 0
        self.h_prev[:] = 0
        self.hs = F(0.0)

    def shift(self, di, dj):
        self.off[0] += int(di)
        self.off[1] += int(dj)
        self.h = shifted(self.h, di, dj)
        self.h_prev = shifted(self.h_prev, di, dj)

    def step(self, records=None, count=None, **settings):
        s = dict(DEFAULTS, **settings)
        acc = splat(self, records, count, s["rho_g"])
        p = (acc.astype(F) * F(2.0 ** -20)).astype(F)
        hs = F(F(s["dt"]) / F(s["substeps"]))
        for _ in range(int(s["substeps"])):
            new = substep(self.h, self.h_prev, p, self.taps, self.dx, hs, s["gravity"], s["damp"], s["edge_damp"],
                          s["border"])
            self.h_prev = self.h
            self.h = new
        self.hs = hs
        return acc

    def sample(self, xz):
        return sample(self, xz)


def shifted(a, di, dj):
    """h'[i, j] = h[i + di, j + dj] where that lies inside, else 0."""
    m = a.shape[0]
    out = np.zeros_like(a)
    i = np.arange(m)
    si, sj = i + int(di), i + int(dj)
    ok_i, ok_j = (si >= 0) & (si < m), (sj >= 0) & (sj < m)
    out[np.ix_(i[ok_j], i[ok_i])] = a[np.ix_(sj[ok_j], si[ok_i])]
    return out


def splat(win, records, count=None, rho_g=9810.0):
    """The accumulators (int64, [j][i]) of the first min(count, rows) records."""
    m = win.m
    acc = np.zeros((m, m), np.int64)
    if records is None:
        return acc
    rec = np.ascontiguousarray(records, F).reshape(-1, 8)
    n = rec.shape[0] if count is None else max(0, min(int(count), rec.shape[0]))
    rec = rec[:n]
    dx = win.dx
    inv = F(F(1.0) / F(F(F(rho_g) * dx) * dx))
    with np.errstate(all="ignore"):
        mm = (rec[:, 5] * inv).astype(F)
        u = ((rec[:, 0] - win.ox()) / dx).astype(F)
        v = ((rec[:, 2] - win.oz()) / dx).astype(F)
        keep = (u >= F(-1.0)) & (u < F(m)) & (v >= F(-1.0)) & (v < F(m))
        mm, u, v = mm[keep], u[keep], v[keep]
        fi, fj = np.floor(u).astype(F), np.floor(v).astype(F)
        fx, fz = (u - fi).astype(F), (v - fj).astype(F)
        i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
        one = F(1.0)
        for di, dj, w in ((0, 0, ((one - fx) * (one - fz))), (1, 0, (fx * (one - fz))), (0, 1, ((one - fx) * fz)),
                          (1, 1, (fx * fz))):
            i, j = i0 + di, j0 + dj
            ok = (i >= 0) & (i < m) & (j >= 0) & (j < m)
            p = (mm * w.astype(F)).astype(F)
            p = np.where(p == p, np.minimum(np.maximum(p, -UNITS), UNITS), F(0.0)).astype(F)
            q = np.trunc((p * UNITS).astype(F)).astype(np.int64)
            np.add.at(acc, (j[ok], i[ok]), q[ok])
    return acc


def _pairs():
    return [(a, b) for a in range(R + 1) for b in range(a + 1)]


def substep(h, h_prev, p, taps, dx, hs, gravity, damp, edge_damp, border):
    """One substep of the contract: the new h from h, h_prev and the pressure head p, all [j][i] float32."""
    m = h.shape[0]
    hs, dx = F(hs), F(dx)
    c = F(F(F(hs * hs) * F(gravity)) / dx)
    hb = F(F(0.5) * hs)
    e = np.zeros((m + 2 * R, m + 2 * R), F)
    e[R:R + m, R:R + m] = (h + p).astype(F)

    def at(di, dj):  # e[i + di, j + dj]
        return e[R + dj:R + dj + m, R + di:R + di + m]

    acc = np.zeros((m, m), F)
    for a, b in _pairs():
        if a == 0:
            s = at(0, 0)
        elif b == 0:
            s = (at(a, 0) + at(-a, 0)) + (at(0, a) + at(0, -a))
        elif a == b:
            s = (at(a, a) + at(-a, -a)) + (at(a, -a) + at(-a, a))
        else:
            s = (((at(a, b) + at(-a, -b)) + (at(a, -b) + at(-a, b))) +
                 ((at(b, a) + at(-b, -a)) + (at(b, -a) + at(-b, a))))
        acc = (acc + (taps[a, b] * s).astype(F)).astype(F)
    i = np.arange(m)
    edge = np.minimum(i, m - 1 - i)
    d = np.minimum(edge[:, None], edge[None, :]).astype(F)
    if border > 0:
        r = (np.maximum(F(border) - d, F(0.0)) / F(border)).astype(F)
    else:
        r = np.zeros((m, m), F)
    alpha = (F(damp) + (F(edge_damp) * (r * r).astype(F)).astype(F)).astype(F)
    b = (hb * alpha).astype(F)
    one, two = F(1.0), F(2.0)
    num = (((two * h).astype(F) - ((one - b).astype(F) * h_prev).astype(F)).astype(F) - (c * acc).astype(F)).astype(F)
    return (num / (one + b).astype(F)).astype(F)


def sample(win, xz):
    """(n, 4) float32: h, dh/dx, dh/dz, dh/dt at the base points xz (n, 2)."""
    xz = np.ascontiguousarray(xz, F).reshape(-1, 2)
    m, dx = win.m, win.dx
    out = np.zeros((xz.shape[0], 4), F)
    with np.errstate(all="ignore"):
        u = ((xz[:, 0] - win.ox()) / dx).astype(F)
        v = ((xz[:, 1] - win.oz()) / dx).astype(F)
        top = F(m - 1)
        ok = (u >= F(0.0)) & (u <= top) & (v >= F(0.0)) & (v <= top)
        u, v = u[ok], v[ok]
        i0 = np.minimum(np.floor(u).astype(np.int64), m - 2)
        j0 = np.minimum(np.floor(v).astype(np.int64), m - 2)
        fx, fz = (u - i0.astype(F)).astype(F), (v - j0.astype(F)).astype(F)

        def bilinear(f):
            f00, f10, f01, f11 = f[j0, i0], f[j0, i0 + 1], f[j0 + 1, i0], f[j0 + 1, i0 + 1]
            x0 = (f00 + (fx * (f10 - f00)).astype(F)).astype(F)
            x1 = (f01 + (fx * (f11 - f01)).astype(F)).astype(F)
            return (x0 + (fz * (x1 - x0)).astype(F)).astype(F), f00, f10, f01, f11

        val, h00, h10, h01, h11 = bilinear(win.h)
        gx = (((h10 - h00) + (fz * ((h11 - h01) - (h10 - h00))).astype(F)).astype(F) / dx).astype(F)
        gz = (((h01 - h00) + (fx * ((h11 - h10) - (h01 - h00))).astype(F)).astype(F) / dx).astype(F)
        if win.hs > 0:
            ht = (bilinear((win.h - win.h_prev).astype(F))[0] / win.hs).astype(F)
        else:
            ht = np.zeros_like(val)
        out[ok] = np.stack([val, gx, gz, ht], axis=1)
    return out
