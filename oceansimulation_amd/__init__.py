"""oceansimulation_amd — MI355X-native (gfx950 HIP) Tessendorf ocean height-field hot path.

Drop-in for the h0 -> h(k,t) -> 2D iFFT path of James51332/OceanSimulation
(Waves::Generator / Waves::FFTCalculator). The compute lives in liboceanfft.so (C ABI,
include/oceanfft.h); this package is its ctypes binding plus a Python mirror of the reference
classes used by the tests and bench.py.
"""
from .capi import (OceanCamera, OceanError, OceanFoamSettings, OceanMarch, OceanSettings, OceanShading,  # noqa: F401
                   OceanSpraySettings, lib)
from .waves import (FFTCalculator, Generator, default_settings, apply_settings,  # noqa: F401
                    default_foam_settings, apply_foam_settings, default_spray_settings, apply_spray_settings)
from .surface import (SprayEmitter, camera_pose, default_camera, default_march, default_shading,  # noqa: F401
                      camera_rays_host)

__all__ = ["FFTCalculator", "Generator", "OceanSettings", "OceanFoamSettings", "OceanSpraySettings", "OceanError",
           "default_settings", "apply_settings", "default_foam_settings", "apply_foam_settings",
           "default_spray_settings", "apply_spray_settings", "SprayEmitter", "OceanCamera", "OceanShading", "OceanMarch",
           "camera_pose", "default_camera", "default_shading", "default_march", "camera_rays_host", "lib"]
