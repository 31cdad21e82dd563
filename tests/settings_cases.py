"""Named settings away from the defaults (TEST INFRASTRUCTURE), for tests/test_settings_space.py.

At the defaults (U_10 = 40, F = 8e5, h = 100, g = 9.8) the spectral peak is at w_p = 0.319 rad/s, a wavelength
of ~600 m, and k h >= 2 pi on every texel of the planes the other tests run (5 .. 251 m): the w <= w_p side of
JONSWAP and of the spreading exponent, tanh / sech of a finite depth and a depth attenuation that is not its
deep-water constant are never evaluated there in a way a wrong value could show. The cases below put a share
of the grid into each of those branches; coverage() measures the shares, and the tests assert them.

Each case is a dict of keyword overrides that both oceansimulation_amd.apply_settings and
oracle.default_settings accept. planeSize is not part of a case: settings(name, n) adds it, scaled by N / 64
from the case's base plane so a texel's (k h, w / w_p) and with it every share below stay what they are at 64.
"""
import numpy as np

DEFAULTS = dict(U_10=40.0, theta_0=25.0, F=800000.0, g=9.8, swell=0.5, h=100.0, planeSize=40.0, spread=0.2)

CASES = {
    "peak": dict(U_10=5.0, F=1e4),                           # w_p = 2.74 rad/s, ~8 m
    "shallow": dict(h=0.2),
    "peak_shallow": dict(U_10=5.0, F=1e4, h=1.0),
    "light_gravity": dict(g=3.71, theta_0=-2.0),
    "no_swell": dict(U_10=5.0, F=1e4, swell=0.0, spread=0.0),  # the pure |cos(theta/2)|^(2s) lobe
    "isotropic": dict(spread=1.0),
}
BASE_PLANE = {"shallow": 101.0}  # metres at N = 64; 40 for every other case (and for the defaults)

# Shares of the grid a case is there for, each >= MIN_SHARE of the texels (coverage()'s keys) ...
REACHES = {
    "peak": ("below_peak", "near_peak"),
    "shallow": ("below_peak", "tanh_series", "tanh_exp", "smoothstep"),
    "peak_shallow": ("below_peak", "near_peak", "tanh_exp", "smoothstep"),
    "light_gravity": (),
    "no_swell": ("below_peak", "near_peak"),
    "isotropic": (),
}
# ... and the cases in deep water at N = 64: tanh(kh) = 1 on every texel, so w is bit-identical to the oracle's
# (the long-time test relies on it)
DEEP = ("peak", "light_gravity", "no_swell", "isotropic")
MIN_SHARE = 0.01


def plane(name, n):
    return BASE_PLANE.get(name, 40.0) * n / 64.0


def settings(name, n):
    """The case's overrides with its plane size at grid size n; name "default" gives the defaults' plane alone."""
    return dict({} if name == "default" else CASES[name], planeSize=plane(name, n))


def coverage(s, n):
    """Shares of the n x n grid's texels (k = 0 left out), in float64, for settings overrides `s` (a dict with
    planeSize): w <= w_p ("below_peak"), k h < 1/8 ("tanh_series", the odd series of tanh), 1/8 <= k h < 2 pi
    ("tanh_exp", 1 - 2 / (1 + e^{2kh})), w sqrt(h / g) < 2 ("smoothstep", depth attenuation not at its constant)
    and |w - w_p| < 0.2 w_p ("near_peak"). Formulas: resources/spectrum.compute:38-44, :60-78, :143."""
    d = dict(DEFAULTS, **s)
    g, h, U, F = (float(d[k]) for k in ("g", "h", "U_10", "F"))
    dk = 2.0 * np.pi / float(d["planeSize"])
    i = (np.arange(n, dtype=np.float64) - n / 2) * dk
    k = np.hypot(i[None, :], i[:, None])
    k = k[k > 0]
    kh = k * h
    w = np.sqrt((g * k + 0.072 / 1000.0 * k ** 3) * np.where(kh >= 2.0 * np.pi, 1.0, np.tanh(kh)))
    w_p = 22.0 * (g * g / (U * F)) ** 0.333
    return dict(below_peak=float(np.mean(w <= w_p)), tanh_series=float(np.mean(kh < 0.125)),
                tanh_exp=float(np.mean((kh >= 0.125) & (kh < 2.0 * np.pi))),
                smoothstep=float(np.mean(w * np.sqrt(h / g) < 2.0)),
                near_peak=float(np.mean(np.abs(w - w_p) < 0.2 * w_p)))
