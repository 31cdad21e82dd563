"""The depth layers and ocean_water_kinematics (include/oceanfft.h, "Depth layers ...") restated in numpy
(TEST INFRASTRUCTURE).

    attenuation       (A_h, A_v) = cosh(k (h - dc)) / cosh(k h), sinh(k (h - dc)) / sinh(k h), dc = min(d, h), per
                      texel, with the fp32 k of numpy_ref.prepare_fft.
                      One deviation from the contract's fp32 exponentials: the factors are evaluated in float64
                      by the stable forms log cosh x = x + log1p(e^{-2x}) - log 2 and log sinh x = x +
                      log(-expm1(-2x)) - log 2 and rounded to float32 once, the same kind of deviation as
                      rates_ref's tanh: the reference is the correctly rounded factor, the kernel's hardware
                      exponentials are judged against it. Both forms give exactly 1 at d == 0 (the two logs are
                      the same number) and A_v gives exactly 0 at d >= h (log sinh 0 = -inf) and at h == 0.
    prepare_height    numpy_ref.prepare_fft's height image with the frame's w: rates_ref's dispersion (a correctly
                      rounded float32 tanh, its docstring) in place of numpy_ref's. With numpy's float32 tanh the
                      four texels at |k| = dk of the 101 m plane get a w one ulp off, 6e-5 rad of phase at
                      t = 1000, and they carry that cascade's largest amplitudes: 2.1e-5 of max |h| between an
                      MI355X's layer 0 and numpy_ref.prepare_fft's transform at t = 1000, against 2.7e-7 with the
                      frame's w. Bit-identical to numpy_ref.prepare_fft wherever the two dispersions agree.
    packed_layer      the two packed images of one layer: prepare_height's lanes (H) and
                      rates_ref.prepare_rate's (Hd), each complex lane times its real factor in float32
    layer_maps        numpy_ref.encode_ifft of both, per depth: [(image 0, image 1)]
    water_kinematics  ocean_water_kinematics on surface_query_ref.surface_query and surface_lod_ref.bilinear,
                      float32 arrays throughout, so every operation rounds as the kernel's unfused fp32
"""
import numpy as np

import numpy_ref as R
import rates_ref
from surface_lod_ref import bilinear
from surface_query_ref import surface_query

F = np.float32


def wavenumbers(s, n: int):
    """k = |kvec| + 1e-6 in float32, as numpy_ref.prepare_fft and rates_ref.prepare_rate form it."""
    s = R.settings_dict(s)
    y, x = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    dk = F(2.0) * R.PI / F(s["planeSize"])
    kx = ((x - F(n) / F(2.0)) * dk).astype(np.float32)
    kz = ((y - F(n) / F(2.0)) * dk).astype(np.float32)
    return (np.sqrt(kx * kx + kz * kz).astype(np.float32) + F(1e-6)).astype(np.float32)


def _log_cosh(x):
    return x + np.log1p(np.exp(-2.0 * x)) - np.log(2.0)


def _log_sinh(x):
    with np.errstate(divide="ignore"):
        return x + np.log(-np.expm1(-2.0 * x)) - np.log(2.0)


def attenuation(k, d, h):
    """(A_h, A_v) as float32 arrays of k's shape."""
    k = np.asarray(k, np.float32).astype(np.float64)
    d, h = float(F(d)), float(F(h))
    dc = min(d, h)
    a, b = k * (h - dc), k * h
    ah = np.exp(_log_cosh(a) - _log_cosh(b))
    if h == 0.0:
        av = np.zeros_like(k)
    else:
        with np.errstate(invalid="ignore"):
            av = np.exp(_log_sinh(a) - _log_sinh(b))
    return ah.astype(np.float32), av.astype(np.float32)


def scale_lanes(img, lane_xy, lane_zw):
    out = img.copy()
    out[..., 0:2] = out[..., 0:2] * lane_xy[..., None]
    out[..., 2:4] = out[..., 2:4] * lane_zw[..., None]
    return out.astype(np.float32)


def prepare_height(s, n: int, h0: np.ndarray):
    """numpy_ref.prepare_fft's height image (H + i dH/dx, dH/dz + i Dx) with rates_ref's dispersion, as
    rates_ref.prepare_rate has it: the same operations on the same float32 values otherwise."""
    s = R.settings_dict(s)
    y, x = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    dk = F(2.0) * R.PI / F(s["planeSize"])
    kx = ((x - F(n) / F(2.0)) * dk).astype(np.float32)
    kz = ((y - F(n) / F(2.0)) * dk).astype(np.float32)
    ln = np.sqrt(kx * kx + kz * kz).astype(np.float32)
    zero = (kx == 0) & (kz == 0)
    with np.errstate(all="ignore"):
        dx = np.where(zero, F(0), kx / ln).astype(np.float32)
    k = (ln + F(1e-6)).astype(np.float32)
    phase = (rates_ref._dispersion(k, F(s["g"]), F(s["h"])) * F(s["time"])).astype(np.float32)
    c, sn = np.cos(phase), np.sin(phase)
    H = (h0[..., 0] + 1j * h0[..., 1]) * (c + 1j * sn) + (h0[..., 2] + 1j * h0[..., 3]) * (c - 1j * sn)
    H = H.astype(np.complex64)
    iH = 1j * H
    A = H + 1j * (kx * iH)
    B = kz * iH + 1j * (dx * iH)
    return np.stack([A.real, A.imag, B.real, B.imag], -1).astype(np.float32)


def packed_layer(s, n: int, h0: np.ndarray, d):
    """image 0 = (A_v * lane xy, A_h * lane zw) of the height packing of Hd,
    image 1 = (A_h * lane xy of the displacement packing of Hd, A_h * lane xy of the height packing of H)."""
    sd = R.settings_dict(s)
    ah, av = attenuation(wavenumbers(sd, n), d, sd["h"])
    rh, rd = rates_ref.prepare_rate(sd, n, h0)
    hp = prepare_height(sd, n, h0)
    img0 = scale_lanes(rh, av, ah)
    img1 = scale_lanes(np.concatenate([rd[..., 0:2], hp[..., 0:2]], -1), ah, ah)
    return img0, img1


def layer_maps(s, n: int, h0: np.ndarray, depths):
    """[(image 0, image 1)] per depth, after EncodeIFFT: image 0 = (vertical velocity, its x-slope, partner,
    d/dt Dx), image 1 = (d/dt Dz, partner, pressure head, its x-slope)."""
    out = []
    for d in depths:
        i0, i1 = packed_layer(s, n, h0, d)
        out.append((R.encode_ifft(i0), R.encode_ifft(i1)))
    return out


def choose_layer(d, depths):
    """(l, f) of the contract for float32 depths d under the surface."""
    D = np.asarray(depths, np.float32)
    L = D.shape[0]
    d = np.asarray(d, np.float32)
    l = np.zeros(d.shape, np.int32)
    f = np.zeros(d.shape, np.float32)
    above = ~(d > D[0])
    below = ~above & (d >= D[L - 1])
    l[below] = L - 1
    mid = ~above & ~below
    if mid.any():
        lm = np.searchsorted(D, d[mid], side="right").astype(np.int32) - 1  # largest index with D[l] <= d
        l[mid] = lm
        f[mid] = ((d[mid] - D[lm]) / (D[lm + 1] - D[lm])).astype(np.float32)
    return l, f


def water_kinematics(oracle, cascades, layers, depths, xyz, iterations, tolerance):
    """cascades: [(height, disp, jac, planeSize, displacement)], layers: per cascade [(image 0, image 1)] per
    depth, xyz (P, 3) world positions -> (P, 12) float32."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    Q = surface_query(oracle, cascades, xyz[:, [0, 2]], iterations, tolerance)
    eta = Q[:, 1]
    s = (eta - xyz[:, 1]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        wet = s > 0
    d = np.where(wet, s, F(0)).astype(np.float32)
    l, f = choose_layer(d, depths)
    L = len(depths)
    blend = f != 0
    px, pz = Q[:, 0].copy(), Q[:, 2].copy()
    u = np.zeros((xyz.shape[0], 4), F)  # ux, uy, uz, P
    rows = np.arange(xyz.shape[0])
    for (hm, dm, _, plane, scale), lay in zip(cascades, layers):
        tu, tv = px / F(plane), pz / F(plane)
        s0 = np.stack([bilinear(lay[j][0], tu, tv) for j in range(L)])  # [layer][P][4]
        s1 = np.stack([bilinear(lay[j][1], tu, tv) for j in range(L)])
        lb = np.minimum(l + 1, L - 1)
        a0, a1, b0, b1 = s0[l, rows], s1[l, rows], s0[lb, rows], s1[lb, rows]
        v0 = np.where(blend[:, None], a0 + f[:, None] * (b0 - a0), a0).astype(np.float32)
        v1 = np.where(blend[:, None], a1 + f[:, None] * (b1 - a1), a1).astype(np.float32)
        sc = F(scale)
        u[:, 0] = u[:, 0] + sc * v0[:, 3]
        u[:, 1] = u[:, 1] + v0[:, 0]
        u[:, 2] = u[:, 2] + sc * v1[:, 0]
        u[:, 3] = u[:, 3] + v1[:, 2]
        H, Dm = bilinear(hm, tu, tv), bilinear(dm, tu, tv)
        px = px + sc * H[:, 3]
        pz = pz + sc * Dm[:, 0]
    out = np.zeros((xyz.shape[0], 12), F)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = Q[:, 0], eta, Q[:, 2], Q[:, 7]
    out[:, 4:8] = u
    out[:, 8], out[:, 9], out[:, 10], out[:, 11] = d, l.astype(np.float32), f, wet.astype(np.float32)
    return out
