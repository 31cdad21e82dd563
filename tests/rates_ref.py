"""The rate maps and the velocity sampler (include/oceanfft.h, "Time derivative of the maps ...")
restated in numpy (TEST INFRASTRUCTURE).

    prepare_rate      numpy_ref.prepare_fft with H(k, t) = a e + b conj(e), e = e^{iwt}, replaced by its time
                      derivative i w (a e - b conj(e)), w and the phase w t in float32 as there; the packing
                      is unchanged, so numpy_ref.encode_ifft of the two images gives d/dt of the eight
                      channels of the maps
                      One deviation from numpy_ref._dispersion: tanh(kh) (used where kh < 2 pi, the longest
                      waves only) is evaluated in float64 and rounded to float32. numpy's float32 tanh is not
                      correctly rounded: at kh = 6.2210755 (|k| = dk of the 101 m plane, h = 100) it returns
                      0.99999207 where tanh is 0.50770 ulp above that, so the correctly rounded value, which
                      the frame's dispersion_evolve and libm give, is 0.99999213. The contract asks for the
                      frame's w; one ulp of w is 6e-5 rad of phase at t = 1000, and those four texels carry
                      the largest amplitudes of that cascade (1.7e-5 of max |dh/dt|, measured on the CPU
                      between the two roundings, against a gate of 1e-5).
    rate_maps         both rate maps of one cascade
    surface_velocity  ocean_surface_velocity with float32 arrays throughout and the taps and weights of
                      surface_lod_ref.bilinear, so every operation rounds as the kernel's unfused fp32
"""
import numpy as np

import numpy_ref as R
from surface_lod_ref import bilinear

F = np.float32


def _dispersion(k, g, h):
    """numpy_ref._dispersion with a correctly rounded float32 tanh (module docstring)."""
    sigma, rho = F(0.072), F(1000.0)
    kh = k * h
    tanh_kh = np.where(kh >= F(2.0) * R.PI, F(1.0), np.tanh(kh.astype(np.float64)).astype(np.float32)).astype(np.float32)
    return np.sqrt((g * k + sigma / rho * k * k * k) * tanh_kh).astype(np.float32)


def prepare_rate(s, n: int, h0: np.ndarray):
    s = R.settings_dict(s)
    y, x = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    dk = F(2.0) * R.PI / F(s["planeSize"])
    kx = ((x - F(n) / F(2.0)) * dk).astype(np.float32)
    kz = ((y - F(n) / F(2.0)) * dk).astype(np.float32)
    ln = np.sqrt(kx * kx + kz * kz).astype(np.float32)
    zero = (kx == 0) & (kz == 0)
    with np.errstate(all="ignore"):
        dx = np.where(zero, F(0), kx / ln).astype(np.float32)
        dz = np.where(zero, F(0), kz / ln).astype(np.float32)
    k = (ln + F(1e-6)).astype(np.float32)
    w = _dispersion(k, F(s["g"]), F(s["h"]))
    phase = (w * F(s["time"])).astype(np.float32)
    e = np.cos(phase) + 1j * np.sin(phase)
    a, b = h0[..., 0] + 1j * h0[..., 1], h0[..., 2] + 1j * h0[..., 3]
    H = (1j * w * (a * e - b * np.conj(e))).astype(np.complex64)
    iH = 1j * H
    A = H + 1j * (kx * iH)
    B = kz * iH + 1j * (dx * iH)
    C = dz * iH + 1j * (-kx * dx * H)
    D = -kz * dz * H + 1j * (-kz * dx * H)
    height = np.stack([A.real, A.imag, B.real, B.imag], -1).astype(np.float32)
    disp = np.stack([C.real, C.imag, D.real, D.imag], -1).astype(np.float32)
    return height, disp


def rate_maps(s, n: int, h0: np.ndarray):
    """(height-rate, displacement-rate) = d/dt (h, dh/dx, dh/dz, Dx), d/dt (Dz, dDx/dx, dDz/dz, dDx/dz)."""
    hp, dp = prepare_rate(s, n, h0)
    return R.encode_ifft(hp), R.encode_ifft(dp)


def surface_velocity(cascades, rates, xz, chain=True):
    """cascades: [(height, disp, jac, planeSize, displacement)], rates: [(height_rate, disp_rate)],
    xz (P, 2) base points -> (P, 8) float32: (displaced x, y, z, 0, velocity x, y, z, 0).
    chain=False drops the grad(field) . u terms (the rate maps sampled along the fixed chain only)."""
    xz = np.ascontiguousarray(xz, F).reshape(-1, 2)
    px, pz = xz[:, 0].copy(), xz[:, 1].copy()
    py = np.zeros_like(px)
    ux, uy, uz = np.zeros_like(px), np.zeros_like(px), np.zeros_like(px)
    for (hm, dm, _, plane, scale), (rhm, rdm) in zip(cascades, rates):
        u, v = px / F(plane), pz / F(plane)
        H, Dm, RH, RD = bilinear(hm, u, v), bilinear(dm, u, v), bilinear(rhm, u, v), bilinear(rdm, u, v)
        s = F(scale)
        if chain:
            vx = s * (RH[:, 3] + (Dm[:, 1] * ux + Dm[:, 3] * uz))
            vy = RH[:, 0] + (H[:, 1] * ux + H[:, 2] * uz)
            vz = s * (RD[:, 0] + (Dm[:, 3] * ux + Dm[:, 2] * uz))
        else:
            vx, vy, vz = s * RH[:, 3], RH[:, 0], s * RD[:, 0]
        px = px + s * H[:, 3]
        py = py + H[:, 0]
        pz = pz + s * Dm[:, 0]
        ux, uy, uz = ux + vx, uy + vy, uz + vz
    out = np.zeros((px.shape[0], 8), F)
    out[:, 0], out[:, 1], out[:, 2] = px, py, pz
    out[:, 4], out[:, 5], out[:, 6] = ux, uy, uz
    return out
