"""The mip pyramid and the footprint-aware surface sampling (include/oceanfft.h, "Mip pyramids ...")
restated in numpy with float32 arrays throughout, so every operation rounds as the kernels' unfused
fp32 does.

    pyramid     L[l+1](x, y) = 0.25f * ((L[l](2x, 2y) + L[l](2x+1, 2y)) + (L[l](2x, 2y+1) + L[l](2x+1, 2y+1)))
    lod_of      r -> (l, f): (0, 0) unless r >= 1; (top, 0) from 2^top; else r's exponent and r / 2^l - 1
    bilinear    GL_LINEAR + GL_REPEAT, the taps and weights of linear_repeat_taps (device/surface_sample.h)
    surface_lod the vertex and fragment stages with A + f * (B - A) between levels l and l + 1
"""
import numpy as np

F = np.float32


def box(level):
    """One halving of an (s, s) or (s, s, C) float32 image, rows y, columns x."""
    level = np.asarray(level, F)
    a, b = level[0::2, 0::2], level[0::2, 1::2]
    c, d = level[1::2, 0::2], level[1::2, 1::2]
    return F(0.25) * ((a + b) + (c + d))


def pyramid(level0):
    """[level 0, level 1, ..., the 1 x 1 level]"""
    levels = [np.ascontiguousarray(level0, F)]
    while levels[-1].shape[0] > 1:
        levels.append(box(levels[-1]))
    return levels


def lod_of(r, top):
    r = np.asarray(r, F)
    l = np.zeros(r.shape, np.int32)
    f = np.zeros(r.shape, F)
    with np.errstate(invalid="ignore"):
        hi = r >= F(1 << top)
        mid = (r >= F(1.0)) & ~hi
    m, e = np.frexp(r[mid])  # r = m * 2^e, m in [0.5, 1)
    l[mid] = e - 1
    f[mid] = m.astype(F) * F(2.0) - F(1.0)  # r * 2^-l - 1, exact
    l[hi] = top
    return l, f


def bilinear(tex, u, v):
    """tex (n, n, C) float32 -> (P, C): w00 t00 + w10 t10 + w01 t01 + w11 t11, summed left to right."""
    n = tex.shape[0]
    tex = tex.reshape(n, n, -1)
    s, t = u * F(n) - F(0.5), v * F(n) - F(0.5)
    fs, ft = np.floor(s), np.floor(t)
    a, b = (s - fs)[:, None], (t - ft)[:, None]
    i0, j0 = fs.astype(np.int64) % n, ft.astype(np.int64) % n
    i1, j1 = (i0 + 1) % n, (j0 + 1) % n
    one = F(1.0)
    w00, w10, w01, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    return w00 * tex[j0, i0] + w10 * tex[j0, i1] + w01 * tex[j1, i0] + w11 * tex[j1, i1]


def sample_blend(pyr, l, f, u, v):
    """Per point: level l[p] of pyr sampled at (u, v), blended towards level l[p] + 1 by f[p] when f != 0."""
    channels = pyr[0].reshape(pyr[0].shape[0], pyr[0].shape[0], -1).shape[2]
    out = np.empty((u.shape[0], channels), F)
    for lev in np.unique(l):
        sel = np.nonzero(l == lev)[0]
        a = bilinear(pyr[lev], u[sel], v[sel])
        nz = f[sel] != 0
        if nz.any():
            b = bilinear(pyr[lev + 1], u[sel][nz], v[sel][nz])
            a[nz] = a[nz] + f[sel][nz][:, None] * (b - a[nz])
        out[sel] = a
    return out


def build_pyramids(cascades):
    """cascades: [(height, disp, jac, planeSize, displacement)] -> [(pyr_h, pyr_d, pyr_j)]"""
    return [(pyramid(h), pyramid(d), pyramid(j)) for h, d, j, _, _ in cascades]


def surface_lod(cascades, xzf, pyramids=None):
    """ocean_surface_sample_lod: xzf (P, 3) = (x, z, footprint) -> (P, 8) float32. pyramids: what
    build_pyramids(cascades) returns (computed once and shared between calls), or None."""
    xzf = np.ascontiguousarray(xzf, F).reshape(-1, 3)
    if pyramids is None:
        pyramids = build_pyramids(cascades)
    n = cascades[0][0].shape[0]
    top = n.bit_length() - 1
    count = len(cascades)
    px, pz, fp = xzf[:, 0].copy(), xzf[:, 1].copy(), xzf[:, 2]
    py = np.zeros_like(px)
    lods = []
    with np.errstate(over="ignore", invalid="ignore"):
        for _, _, _, plane, _ in cascades:
            lods.append(lod_of((fp * F(n)) / F(plane), top))
    # vertex stage: cascade c samples at the position cascades < c displaced
    for (ph, pd, _), (_, _, _, plane, scale), (l, f) in zip(pyramids, cascades, lods):
        u, v = px / F(plane), pz / F(plane)
        h, d = sample_blend(ph, l, f, u, v), sample_blend(pd, l, f, u, v)
        px = px + F(scale) * h[:, 3]
        py = py + h[:, 0]
        pz = pz + F(scale) * d[:, 0]
    # fragment stage at the displaced position
    acc = [np.zeros_like(px) for _ in range(4)]
    jac = np.zeros_like(px)
    for (ph, pd, pj), (_, _, _, plane, scale), (l, f) in zip(pyramids, cascades, lods):
        u, v = px / F(plane), pz / F(plane)
        h, d, j = sample_blend(ph, l, f, u, v), sample_blend(pd, l, f, u, v), sample_blend(pj, l, f, u, v)
        jac = jac + j[:, 0] / F(count)
        acc[0] = acc[0] + h[:, 1]
        acc[1] = acc[1] + d[:, 1] * F(scale)
        acc[2] = acc[2] + h[:, 2]
        acc[3] = acc[3] + d[:, 2] * F(scale)
    one = F(1.0)
    sx, sz = acc[0] / (one + acc[1]), acc[2] / (one + acc[3])
    nx, ny, nz = -sx, np.ones_like(sx), -sz
    length = np.sqrt(nx * nx + ny * ny + nz * nz)
    out = np.empty((px.shape[0], 8), F)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = px, py, pz, jac
    out[:, 4], out[:, 5], out[:, 6], out[:, 7] = nx / length, ny / length, nz / length, fp
    return out
