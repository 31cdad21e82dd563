"""oceansimulation_amd — MI355X-native (gfx950 HIP) Tessendorf ocean height-field hot path.

Drop-in for the h0 -> h(k,t) -> 2D iFFT path of James51332/OceanSimulation
(Waves::Generator / Waves::FFTCalculator). The compute lives in liboceanfft.so (C ABI,
include/oceanfft.h); this package is its ctypes binding plus a Python mirror of the reference
classes used by the tests and bench.py.
"""
from .capi import (OceanCamera, OceanCameraLayers, OceanError, OceanFoamDepositSettings, OceanFoamSettings, OceanMarch,  # noqa: F401
                   OceanHullStepSettings, OceanParticleSettings, OceanSettings, OceanShading, OceanSpraySettings,
                   OceanWakeSettings, lib)
from .waves import (FFTCalculator, Generator, default_settings, apply_settings,  # noqa: F401
                    default_foam_settings, apply_foam_settings, default_spray_settings, apply_spray_settings,
                    default_particle_settings, apply_particle_settings, default_foam_deposit_settings,
                    apply_foam_deposit_settings)
from .surface import (SprayEmitter, SprayParticles, camera_pose, default_camera, default_march,  # noqa: F401
                      default_shading, default_camera_layers, camera_rays_host)
from .wake import Wake, default_wake_settings, apply_wake_settings  # noqa: F401

__all__ = ["FFTCalculator", "Generator", "OceanSettings", "OceanFoamSettings", "OceanSpraySettings",
           "OceanParticleSettings", "OceanFoamDepositSettings", "OceanHullStepSettings", "OceanError",
           "default_settings", "apply_settings", "default_foam_settings", "apply_foam_settings",
           "default_spray_settings", "apply_spray_settings", "default_particle_settings", "apply_particle_settings",
           "default_foam_deposit_settings", "apply_foam_deposit_settings",
           "SprayEmitter", "SprayParticles", "OceanCamera", "OceanShading", "OceanMarch", "OceanCameraLayers",
           "camera_pose", "default_camera", "default_shading", "default_march", "default_camera_layers",
           "camera_rays_host", "Wake", "OceanWakeSettings", "default_wake_settings", "apply_wake_settings", "lib"]
