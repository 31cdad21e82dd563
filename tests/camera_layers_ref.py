"""ocean_camera_render_layers' contract (include/oceanfft.h) restated in numpy float32 on top of
tests/camera_ref.py (the water pass without foam), tests/foam_ref.py (the foam's taps) and the ray formula.

    water      camera_ref.render, then at the hits the foam at V.xz, w, fc and col' = col*(1 - w) + fc*w under the
               same fog factor f (exp in float64, rounded once)
    project    the spray pass's projection of world points: z, ci, cj, half and the cull
    splat      key = min over the records that pass the depth test of (bits(z) << 32 | r), hits = their number:
               integers, so the order of the records does not matter; a Python loop over the records
    composite  a, fs (exp in float64, rounded once), sc and out = base*(1 - a) + sc*a
Every array is float32, so each operation rounds as the kernels' unfused fp32 does.
"""
import numpy as np

import camera_ref as CR
import foam_ref as FR
import raycast_ref as RR

f32 = np.float32
NO_RECORD = np.uint32(0xFFFFFFFF)


def _dot3(e, v):
    return (e[:, 0] * v[0] + e[:, 1] * v[1]) + e[:, 2] * v[2]


def project(cam, width, height, pos, radius=0.0, max_half=0):
    """pos (n, 3) -> dict of (n,) arrays: z, ci, cj (float32, floorf'ed), half (int), keep (not culled)."""
    w, h = int(width), int(height)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    T = f32(cam.tan_half_fov_y)
    aspect = f32(w) / f32(h)
    e = pos - CR._vec(cam.position)[None, :]
    with np.errstate(all="ignore"):
        z = _dot3(e, CR._vec(cam.forward))
        x = _dot3(e, CR._vec(cam.right))
        y = _dot3(e, CR._vec(cam.up))
        depth_ok = (z >= f32(cam.near_plane)) & (z <= f32(cam.far_plane))
        ci = np.floor(((x / (z * (aspect * T))) + f32(1)) * (f32(0.5) * f32(w)))
        cj = np.floor((f32(1) - (y / (z * T))) * (f32(0.5) * f32(h)))
        hf = np.minimum(np.floor(f32(radius) / (z * ((f32(2) * T) / f32(h)))), f32(max_half))
        half = np.where(np.isnan(hf), f32(0), hf).astype(np.int64)
        fh = half.astype(f32)
        inside = (ci >= -fh) & (ci <= (f32(w - 1) + fh)) & (cj >= -fh) & (cj <= (f32(h - 1) + fh))
    assert z.dtype == f32 and ci.dtype == f32 and cj.dtype == f32
    return dict(z=z, ci=ci, cj=cj, half=half, keep=depth_ok & inside)


def foam_weight(foam, layers):
    """w of the contract for the foam values `foam` (float32)."""
    with np.errstate(all="ignore"):
        w = np.minimum(np.maximum((foam - f32(layers.foam_lo)) / (f32(layers.foam_hi) - f32(layers.foam_lo)), f32(0)),
                       f32(1))
        w = (w * w) * (f32(3) - f32(2) * w)
        return w * f32(layers.foam_opacity)


def splat(cam, layers, width, height, aux, records, n):
    """key (h*w,) uint64 and hits (h*w,) uint32 of records[:n] against the water pass's aux (h, w, 4)."""
    w, h = int(width), int(height)
    key = np.full(w * h, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    hits = np.zeros(w * h, np.uint32)
    if n <= 0:
        return key, hits
    rec = np.ascontiguousarray(records).reshape(-1, 8)[:n].view(f32)
    pr = project(cam, w, h, rec[:, :3], layers.spray_radius, layers.spray_max_half)
    status, depth = aux.reshape(-1, 4)[:, 3], aux.reshape(-1, 4)[:, 1]
    for r in np.nonzero(pr["keep"])[0]:
        z, half = pr["z"][r], int(pr["half"][r])
        i0, j0 = int(pr["ci"][r]), int(pr["cj"][r])
        k = (np.uint64(z.view(np.uint32)) << np.uint64(32)) | np.uint64(r)
        for b in range(max(j0 - half, 0), min(j0 + half, h - 1) + 1):
            for a in range(max(i0 - half, 0), min(i0 + half, w - 1) + 1):
                q = b * w + a
                if status[q] != 0 or z < depth[q]:
                    key[q] = min(key[q], k)
                    hits[q] += np.uint32(1)
    return key, hits


def render(oracle, cascades, cam, shading, march, layers, width, height, bounds=None, pyramids=None, foams=None,
           records=None, count=None):
    """camera_ref.render's arguments, then foams: one (n, n) map per cascade (read when layers.foam_opacity > 0),
    records: (m, 8) of 4-byte values or None, count: the device count or None (all m).
    Returns camera_ref.render's dict for the water pass without foam under "water", and: image, aux, aux2
    (h, w, 4) float32 (aux2's slots 2, 3 are uint32 bits), image8, and flat per pixel: foam, w, fc, colp (col'),
    f, sky_d, base (the water pass's pixel), status, z, key, hits, a, fs, s (spray colour * light colour), sc."""
    w, h = int(width), int(height)
    n_pix = w * h
    water = CR.render(oracle, cascades, cam, shading, march, w, h, bounds=bounds, pyramids=pyramids)
    hit = water["status"] == RR.HIT
    col, f, sky_d = water["col"], water["f"], water["sky_d"]
    foam = np.zeros(n_pix, f32)
    wgt = np.zeros(n_pix, f32)
    fc = np.zeros((n_pix, 3), f32)
    colp = col.copy()
    if f32(layers.foam_opacity) > 0:
        L, _, _ = CR.host_constants(shading)
        with np.errstate(all="ignore"):
            fo = FR._foam_slot(cascades, foams, water["P"][:, 0].copy(), water["P"][:, 2].copy())
            wg = foam_weight(fo, layers)
            diffuse = np.maximum(CR._dot(water["normal"], L[None, :]), f32(0)) * f32(0.3)
            lit = (diffuse + f32(0.5))[:, None] * CR._vec(layers.foam_color)[None, :]
            mixed = col * (f32(1) - wg)[:, None] + lit * wg[:, None]
        foam = np.where(hit, fo, f32(0)).astype(f32)
        wgt = np.where(hit, wg, f32(0)).astype(f32)
        fc = np.where(hit[:, None], lit, f32(0)).astype(f32)
        colp = np.where(hit[:, None], mixed, f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        fogged = colp * (f32(1) - f)[:, None] + sky_d * f[:, None]
    base = np.where(hit[:, None], fogged, sky_d).astype(f32)
    aux = water["aux"]
    key = np.full(n_pix, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    hits = np.zeros(n_pix, np.uint32)
    if records is not None and len(records):
        m = np.ascontiguousarray(records).reshape(-1, 8).shape[0]
        n = m if count is None else min(int(count), m)
        key, hits = splat(cam, layers, w, h, aux, records, n)
    covered = hits > 0
    zs = np.where(covered, (key >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    rid = np.where(covered, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), NO_RECORD).astype(np.uint32)
    with np.errstate(all="ignore"):
        a = np.minimum(hits.astype(f32) * f32(layers.spray_opacity), f32(1))
        arg = -((zs - f32(shading.fog_begin)) * f32(shading.fog_density))
        fs = np.maximum(f32(1) - np.exp(arg.astype(np.float64)).astype(f32), f32(0))
        s = (CR._vec(layers.spray_color) * CR._vec(shading.light_color))[None, :].repeat(n_pix, 0)
        sc = s * (f32(1) - fs)[:, None] + sky_d * fs[:, None]
        mixed = base * (f32(1) - a)[:, None] + sc * a[:, None]
    out = np.where(covered[:, None], mixed, base).astype(f32)
    a = np.where(covered, a, f32(0)).astype(f32)
    fs = np.where(covered, fs, f32(0)).astype(f32)
    image = np.concatenate([out, np.ones((n_pix, 1), f32)], 1)
    aux2 = np.stack([foam, zs, hits.view(f32), rid.view(f32)], 1)
    assert image.dtype == f32 and aux2.dtype == f32 and base.dtype == f32
    return dict(water=water, image=image.reshape(h, w, 4), aux=aux, aux2=aux2.reshape(h, w, 4),
                image8=CR.to_bytes(out).reshape(h, w, 4), foam=foam, w=wgt, fc=fc, colp=colp, f=f, sky_d=sky_d,
                base=base, status=water["status"], z=water["z"], key=key, hits=hits, a=a, fs=fs, s=s, sc=sc)
