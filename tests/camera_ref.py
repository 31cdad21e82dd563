"""ocean_camera_render's contract (include/oceanfft.h) restated in numpy float32 on top of the ray march of
tests/raycast_ref.py, the oracle's forward map and the mip-pyramid sampling of tests/surface_lod_ref.py.

    rays     the header's ray formula (ocean_camera_rays writes exactly these)
    march    raycast_ref.raycast on those rays: status, t, the base point p of the final evaluation; V(p) and
             the fragment stage are oracle.surface_points(p) (bit for bit), or with lod_scale > 0 the
             fragment stage of surface_lod_ref at V.xz with the pixel's footprint
    shade    sky, water and fog in any float type: float32 is the contract (every operation rounds as the
             kernel's unfused fp32 does; exp is evaluated in float64 and rounded once), float64 is the
             reading of the same formulas that tests/test_camera.py measures the fp32 error against
np.minimum / np.maximum return NaN when either operand is NaN, as the contract's min / max do.
"""
import numpy as np

import raycast_ref as RR
import surface_lod_ref as SL

f32 = np.float32
DEG = 0.0174533  # waveShader.glsl:39


def _vec(a, dtype=f32):
    return np.array([a[0], a[1], a[2]], dtype)


def camera_rays(cam, width, height):
    """((h * w, 8) float32 rays, (h * w,) float32 len): row 0 is the top row, x fastest."""
    w, h = int(width), int(height)
    T = f32(cam.tan_half_fov_y)
    aspect = f32(w) / f32(h)
    i = np.tile(np.arange(w, dtype=f32), h)
    j = np.repeat(np.arange(h, dtype=f32), w)
    x = (((f32(2) * (i + f32(0.5))) / f32(w)) - f32(1)) * (aspect * T)
    y = (f32(1) - ((f32(2) * (j + f32(0.5))) / f32(h))) * T
    length = np.sqrt((x * x + y * y) + f32(1))
    right, up, fwd, pos = _vec(cam.right), _vec(cam.up), _vec(cam.forward), _vec(cam.position)
    rays = np.zeros((w * h, 8), f32)
    for k in range(3):
        rays[:, k] = pos[k]
        rays[:, 4 + k] = ((x * right[k] + y * up[k]) + fwd[k]) / length
    rays[:, 3] = f32(cam.near_plane) * length
    rays[:, 7] = f32(cam.far_plane) * length
    assert rays.dtype == f32 and length.dtype == f32
    return rays, length


def host_constants(shading, dtype=f32):
    """(L, cthr, cfade): evaluated in double and, for float32, rounded once."""
    l = np.array([float(v) for v in shading.light_direction], np.float64)
    L = l / np.sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2])
    sva, sfa = float(f32(shading.sun_view_angle)), float(f32(shading.sun_falloff_angle))
    cthr = np.cos(sva * DEG)
    cfade = np.cos((sva + max(sfa, 0.01)) * DEG)
    return L.astype(dtype), dtype(cthr), dtype(cfade)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def sky(v, shading, F=f32):
    """sky(v) for directions v (n, 3) of type F -> (n, 3)."""
    L, cthr, cfade = host_constants(shading, F)
    sky_c, light_c = _vec(shading.sky_color, F), _vec(shading.light_color, F)
    u = _normalize(v)
    s = _dot(L[None, :], u)
    e = np.minimum(np.maximum((s - cfade) / (cthr - cfade), F(0)), F(1))
    w = (e * e) * (F(3) - F(2) * e)
    w = w * (w * w)
    m = F(0.8) - u[:, 1] / F(0.8)
    m = m * m
    box = sky_c[None, :] * (F(1) - m)[:, None] + light_c[None, :] * m[:, None]
    return (F(1) - w)[:, None] * box + (F(2) * w)[:, None] * light_c[None, :]


def shade(P, n, d, z, hit, position, shading, F=f32):
    """The header's sky / water / fog for pixels with surface point P (n, 3), normal n, ray direction d, view
    depth z and hit mask, evaluated in type F. Returns dict(out, col, sky_d, f), col and f zero off the hits."""
    P, n, d, z = (np.asarray(a, F) for a in (P, n, d, z))
    L, _, _ = host_constants(shading, F)
    wave_c, scatter_c = _vec(shading.wave_color, F), _vec(shading.scatter_color, F)
    with np.errstate(all="ignore"):
        sky_d = sky(d, shading, F)
        I = -_normalize(_vec(position, F)[None, :] - P)
        k = F(2) * _dot(n, I)
        r = I - k[:, None] * n
        diffuse = np.maximum(_dot(n, L[None, :]), F(0)) * F(0.3)
        sp = np.maximum(_dot(r, L[None, :]), F(0))
        for _ in range(5):
            sp = sp * sp
        specular = sp * F(0.5)
        scatter = np.maximum(P[:, 1] * F(0.1), F(0))
        light = (diffuse + F(0.5)) + specular
        col = ((light[:, None] * wave_c[None, :]) * sky(r, shading, F)) + scatter[:, None] * scatter_c[None, :]
        arg = -((z - F(shading.fog_begin)) * F(shading.fog_density))
        f = np.maximum(F(1) - np.exp(arg.astype(np.float64)).astype(F), F(0))
        out = col * (F(1) - f)[:, None] + sky_d * f[:, None]
    hit = np.asarray(hit, bool)
    out = np.where(hit[:, None], out, sky_d)
    col = np.where(hit[:, None], col, F(0))
    f = np.where(hit, f, F(0))
    assert out.dtype == F
    return dict(out=out, col=col, sky_d=sky_d, f=f)


def to_bytes(rgb):
    """image8: per channel !(c > 0) ? 0 : (uint8)(min(c, 1) * 255 + 0.5), alpha 255."""
    rgb = np.asarray(rgb, f32)
    with np.errstate(invalid="ignore"):
        q = np.minimum(rgb, f32(1)) * f32(255) + f32(0.5)
        b = np.where(rgb > 0, q, f32(0)).astype(np.uint8)
    return np.concatenate([b, np.full((rgb.shape[0], 1), 255, np.uint8)], 1)


def fragment_lod(cascades, pyramids, vx, vz, footprint):
    """ocean_surface_sample_lod's fragment stage at (vx, vz) -> (n, 4): normal, jacobian (surface_lod_ref's)."""
    F = f32
    n = cascades[0][0].shape[0]
    top = n.bit_length() - 1
    count = len(cascades)
    acc = [np.zeros_like(vx) for _ in range(4)]
    jac = np.zeros_like(vx)
    with np.errstate(over="ignore", invalid="ignore"):
        for (ph, pd, pj), (_, _, _, plane, scale) in zip(pyramids, cascades):
            l, f = SL.lod_of((footprint * F(n)) / F(plane), top)
            u, v = vx / F(plane), vz / F(plane)
            h, d, j = SL.sample_blend(ph, l, f, u, v), SL.sample_blend(pd, l, f, u, v), SL.sample_blend(pj, l, f, u, v)
            jac = jac + j[:, 0] / F(count)
            acc[0] = acc[0] + h[:, 1]
            acc[1] = acc[1] + d[:, 1] * F(scale)
            acc[2] = acc[2] + h[:, 2]
            acc[3] = acc[3] + d[:, 2] * F(scale)
        sx, sz = acc[0] / (F(1) + acc[1]), acc[2] / (F(1) + acc[3])
        nx, ny, nz = -sx, np.ones_like(sx), -sz
        length = np.sqrt(nx * nx + ny * ny + nz * nz)
    return np.stack([nx / length, ny / length, nz / length, jac], 1).astype(F)


def render(oracle, cascades, cam, shading, march, width, height, bounds=None, pyramids=None):
    """cascades: [(height, disp, jac, planeSize, displacement)]; bounds: (count, 18) or None (the maps' own);
    pyramids: surface_lod_ref.build_pyramids(cascades) or None, used when cam.lod_scale > 0.
    Returns dict: image (h, w, 4) float32, aux (h, w, 4) float32, image8 (h, w, 4) uint8, and per pixel
    (flat, row-major) rays, hits (the raycast rows), status, z, f, col, sky_d, P, normal."""
    w, h = int(width), int(height)
    rays, length = camera_rays(cam, w, h)
    hits = RR.raycast(oracle, cascades, rays, step=march.step, max_steps=march.max_steps, refine=march.refine,
                      iterations=march.iterations, tolerance=march.tolerance, slope=march.slope, pad=march.pad,
                      bounds=bounds)
    status = hits[:, 12].astype(int)
    outside = status == RR.OUTSIDE
    t = hits[:, 3]
    z = (t / length).astype(f32)
    base = np.ascontiguousarray(hits[:, [8, 10]])
    V = oracle.surface_points(cascades, base)[:, :3]  # the final evaluation's V(p)
    normal, jac = hits[:, 4:7].copy(), hits[:, 7].copy()
    lod = f32(cam.lod_scale)
    if lod > 0:
        if pyramids is None:
            pyramids = SL.build_pyramids(cascades)
        footprint = lod * (z * ((f32(2) * f32(cam.tan_half_fov_y)) / f32(h)))
        frag = fragment_lod(cascades, pyramids, V[:, 0].copy(), V[:, 2].copy(), footprint.astype(f32))
        normal, jac = frag[:, :3], frag[:, 3]
        jac = np.where(outside, f32(0), jac)
    hit = status == RR.HIT
    s = shade(V, normal, rays[:, 4:7], z, hit, cam.position, shading, f32)
    image = np.concatenate([s["out"], np.ones((w * h, 1), f32)], 1)
    aux = np.stack([t, z, jac, status.astype(f32)], 1).astype(f32)
    aux[outside] = (0.0, 0.0, 0.0, 1.0)
    return dict(image=image.reshape(h, w, 4), aux=aux.reshape(h, w, 4), image8=to_bytes(s["out"]).reshape(h, w, 4),
                rays=rays, hits=hits, status=status, z=z, f=s["f"], col=s["col"], sky_d=s["sky_d"], P=V,
                normal=normal)
