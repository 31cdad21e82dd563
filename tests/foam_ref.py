"""Persistent foam (include/oceanfft.h, "Persistent foam ...") restated in numpy with float32 arrays
throughout, so every operation rounds as the kernels' unfused fp32 does.

    step        a = (float) exp(-(double)decay * (double)dt);  s = max(bias - J, 0) * gain
                t = F * a + s * dt;  F' = min(t, 1)
                counts = (#(bias - J > 0), #(F' >= level), #(t >= 1))
    sample_foam ocean_surface_sample's eight floats from the oracle, slot 7 = sum_c tap_c(F_c) / count with the
                fragment stage's taps: GL_LINEAR + GL_REPEAT at the displaced position (slots 0 and 2)
"""
import math

import numpy as np

from surface_lod_ref import bilinear

F = np.float32


def decay_factor(decay, dt):
    return F(math.exp(-float(F(decay)) * float(F(dt))))


def step(foam, jac, bias, gain, decay, level, dt):
    """One ocean_generator_advance_foam of one cascade: (F', int64 (breaking, covered, saturated))."""
    foam, jac = np.asarray(foam, F), np.asarray(jac, F)
    a = decay_factor(decay, dt)
    d = F(bias) - jac
    s = np.maximum(d, F(0.0)) * F(gain)
    t = foam * a + s * F(dt)
    out = np.minimum(t, F(1.0))
    counts = np.array([np.count_nonzero(d > 0), np.count_nonzero(out >= F(level)), np.count_nonzero(t >= F(1.0))],
                      np.int64)
    return out, counts


def _foam_slot(cascades, foams, px, pz):
    foam = np.zeros_like(px)
    count = len(cascades)
    for (_, _, _, plane, _), fm in zip(cascades, foams):
        u, v = px / F(plane), pz / F(plane)
        foam = foam + bilinear(np.ascontiguousarray(fm, F), u, v)[:, 0] / F(count)
    return foam


def sample_foam(oracle, cascades, foams, xz):
    """cascades: [(height, disp, jac, planeSize, displacement)] as oracle.surface_points takes them; foams: one
    (n, n) map per cascade; xz (P, 2) -> (P, 8)."""
    out = oracle.surface_points(cascades, np.ascontiguousarray(xz, F).reshape(-1, 2)).copy()
    out[:, 7] = _foam_slot(cascades, foams, out[:, 0].copy(), out[:, 2].copy())
    return out


def sample_plane_foam(oracle, cascades, foams, camera, res):
    out = oracle.surface_plane(cascades, camera, res).copy()
    out[:, 7] = _foam_slot(cascades, foams, out[:, 0].copy(), out[:, 2].copy())
    return out
