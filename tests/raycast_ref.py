"""ocean_surface_raycast's contract (include/oceanfft.h) restated in numpy float32 on top of the oracle's
forward map: oracle.surface_points is V(p) and the fragment stage bit for bit, so no sampler is restated.
The bounds are np.min / np.max of the maps. Every ray is the header's small state machine (first
evaluation, march, bisection, final evaluation); the rays that still run are evaluated together, one
E(t) per round, exactly one oracle call per fixed-point step.

    slab:   ylo = sum bounds_c[0] - pad, yhi = sum bounds_c[1] + pad          (in pair order, fp32)
    clip:   t0, t1 from (tmin, tmax) and the slab; OUTSIDE when the ray misses it (or NaN)
    E(t):   q = (ox + t dx, oz + t dz); p = q + off; the query's fixed point from p; off = p - q;
            g = (oy + t dy) - V.y
    march:  tb = min(ta + max(step, |ga| * inv), t1) until the sign of g changes (HIT), tb >= t1 (EXIT)
            or max_steps (STEP_LIMIT); refine: `refine` bisections, then the secant point; final E(t)
np.minimum / np.maximum return NaN when either operand is NaN, as the contract's min / max do.
"""
import numpy as np

f32 = np.float32
HIT, OUTSIDE, EXIT, STEP_LIMIT = 0, 1, 2, 3
_FIRST, _MARCH, _REFINE, _FINAL, _DONE = range(5)


def map_bounds(cascades):
    """(count, 18) float32: per cascade (min, max) of heightMap x, y, z, w, displacementMap x, y, z, w, jacobian."""
    out = np.zeros((len(cascades), 18), f32)
    for i, cas in enumerate(cascades):
        h, d, j = cas[0], cas[1], cas[2]
        chans = [h[..., c] for c in range(4)] + [d[..., c] for c in range(4)] + [j]
        for c, img in enumerate(chans):
            out[i, 2 * c] = np.min(img)
            out[i, 2 * c + 1] = np.max(img)
    return out


def slab(bounds, pad):
    ylo, yhi = f32(0.0), f32(0.0)
    for row in np.asarray(bounds, f32).reshape(-1, 18):
        ylo = f32(ylo + row[0])
        yhi = f32(yhi + row[1])
    return f32(ylo - f32(pad)), f32(yhi + f32(pad))


def raycast(oracle, cascades, rays, step=0.25, max_steps=256, refine=10, iterations=4, tolerance=1e-3,
            slope=np.inf, pad=0.0, bounds=None, with_stats=False):
    """cascades: [(height, disp, jac, planeSize, displacement)] as oracle.surface_points takes them; rays:
    (n, 8) (ox, oy, oz, tmin, dx, dy, dz, tmax); bounds: (count, 18), default map_bounds(cascades).
    Returns (n, 16) float32, and with with_stats also dict(evals, fp_steps): evaluations E and
    fixed-point steps (vertex stages beyond the first of an evaluation) over all rays."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    n = rays.shape[0]
    ox, oy, oz, tmin = (rays[:, k].copy() for k in range(4))
    dx, dy, dz, tmax = (rays[:, k].copy() for k in range(4, 8))
    step, tol, slope = f32(step), f32(tolerance), f32(slope)
    ylo, yhi = slab(map_bounds(cascades) if bounds is None else bounds, pad)
    stats = dict(evals=0, fp_steps=0)
    with np.errstate(all="ignore"):
        a, b = (ylo - oy) / dy, (yhi - oy) / dy
        sloped = dy != 0  # NaN too, as in C
        t0 = np.where(sloped, np.maximum(tmin, np.minimum(a, b)), tmin).astype(f32)
        t1 = np.where(sloped, np.minimum(tmax, np.maximum(a, b)), tmax).astype(f32)
        outside = (~sloped & ~((ylo <= oy) & (oy <= yhi))) | ~(t0 <= t1)
        if np.isinf(slope):
            inv = np.zeros(n, f32)
        else:
            inv = (f32(1.0) / (np.abs(dy) + slope * np.sqrt(dx * dx + dz * dz))).astype(f32)

    phase = np.where(outside, _DONE, _FIRST)
    status = np.where(outside, OUTSIDE, HIT)
    steps = np.zeros(n, np.int64)
    left = np.full(n, int(refine), np.int64)
    below = np.zeros(n, bool)
    te, ta, tb = t0.copy(), t0.copy(), t0.copy()
    ga, gb, g = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    off, q, p = np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.zeros((n, 2), f32)
    V = np.zeros((n, 8), f32)

    def evaluate(idx):
        t = te[idx]
        qi = np.stack([ox[idx] + t * dx[idx], oz[idx] + t * dz[idx]], 1).astype(f32)
        pi = (qi + off[idx]).astype(f32)
        Vi = oracle.surface_points(cascades, np.ascontiguousarray(pi))
        active = np.ones(idx.size, bool)
        for _ in range(int(iterations)):
            r = (qi - Vi[:, [0, 2]]).astype(f32)
            active &= ~(np.maximum(np.abs(r[:, 0]), np.abs(r[:, 1])) <= tol)
            if not active.any():
                break
            pi[active] = (pi[active] + r[active]).astype(f32)
            Vi[active] = oracle.surface_points(cascades, np.ascontiguousarray(pi[active]))
            stats["fp_steps"] += int(active.sum())
        stats["evals"] += int(idx.size)
        off[idx] = (pi - qi).astype(f32)
        q[idx], p[idx], V[idx] = qi, pi, Vi
        g[idx] = ((oy[idx] + t * dy[idx]) - Vi[:, 1]).astype(f32)

    with np.errstate(all="ignore"):
        while True:
            idx = np.nonzero(phase != _DONE)[0]
            if idx.size == 0:
                break
            evaluate(idx)
            act = phase != _DONE
            first, march, ref, fin = (act & (phase == k) for k in (_FIRST, _MARCH, _REFINE, _FINAL))
            neg = g <= 0
            # the first evaluation
            ga[first] = g[first]
            below[first] = neg[first]
            phase[first] = _MARCH
            advance = first.copy()  # max_steps >= 1
            # a marching step
            gb[march] = g[march]
            steps[march] += 1
            cross = march & (neg != below)
            cont = march & ~cross
            phase[cross] = _REFINE
            ta[cont] = tb[cont]
            ga[cont] = gb[cont]
            ex = cont & (tb >= t1)
            lim = cont & ~ex & (steps == int(max_steps))
            status[ex], status[lim] = EXIT, STEP_LIMIT
            for m in (ex, lim):
                phase[m] = _FINAL
                te[m] = ta[m]
            advance |= cont & ~ex & ~lim
            # a bisection
            same = ref & (neg == below)
            other = ref & ~same
            ta[same], ga[same] = te[same], g[same]
            tb[other], gb[other] = te[other], g[other]
            left[ref] -= 1
            # the final evaluation is done
            phase[fin] = _DONE
            # what comes next
            nxt = np.minimum(ta + np.maximum(step, np.abs(ga) * inv), t1).astype(f32)
            tb[advance] = nxt[advance]
            te[advance] = nxt[advance]
            bis = act & (phase == _REFINE)
            mid = bis & (left > 0)
            end = bis & ~mid
            te[mid] = (f32(0.5) * (ta + tb)).astype(f32)[mid]
            te[end] = (ta + (tb - ta) * (ga / (ga - gb))).astype(f32)[end]
            phase[end] = _FINAL

        out = np.zeros((n, 16), f32)
        t = te
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = ox + t * dx, oy + t * dy, oz + t * dz, t
        out[:, 4:7] = V[:, 4:7]
        out[:, 7] = V[:, 3]
        out[:, 8], out[:, 9], out[:, 10] = p[:, 0], V[:, 1], p[:, 1]
        out[:, 11] = np.maximum(np.abs(q[:, 0] - V[:, 0]), np.abs(q[:, 1] - V[:, 2]))
        out[:, 12], out[:, 13], out[:, 14], out[:, 15] = status, below, steps, g
        out[outside] = 0.0
        out[outside, 12] = f32(OUTSIDE)
    return (out, stats) if with_stats else out
