"""ctypes binding of liboceanfft.so — every entry point declared in include/oceanfft.h.

The library is the product path (HIP kernels for gfx950). There is no CPU fallback: if the
shared object is missing, `lib()` raises, and every compute call fails loudly without a GPU.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboceanfft.so")

OCEAN_OK = 0
OCEAN_ERR_INVALID = 1
OCEAN_ERR_HIP = 2
OCEAN_ERR_NO_DEVICE = 3
OCEAN_ERR_OOM = 4
OCEAN_ERR_TIMEOUT = 5
OCEAN_MAX_CASCADES = 64
OCEAN_COMM_ID_BYTES = 128
OCEAN_PEER_HANDLE_BYTES = 256


class OceanSettings(ctypes.Structure):
    """ocean_settings == Waves::GeneratorSettings (reference src/Generator.h:12-30), 64 bytes."""

    _fields_ = [
        ("seed", ctypes.c_int32 * 2),
        ("U_10", ctypes.c_float),
        ("theta_0", ctypes.c_float),
        ("F", ctypes.c_float),
        ("g", ctypes.c_float),
        ("swell", ctypes.c_float),
        ("h", ctypes.c_float),
        ("displacement", ctypes.c_float),
        ("time", ctypes.c_float),
        ("planeSize", ctypes.c_float),
        ("scale", ctypes.c_float),
        ("spread", ctypes.c_float),
        ("boundWavelength", ctypes.c_int32),
        ("wavelengthMin", ctypes.c_float),
        ("wavelengthMax", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanSettings) == 64


class OceanFoamSettings(ctypes.Structure):
    """ocean_foam_settings: one cascade's persistent-foam parameters, 16 bytes."""

    _fields_ = [
        ("bias", ctypes.c_float),
        ("gain", ctypes.c_float),
        ("decay", ctypes.c_float),
        ("level", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanFoamSettings) == 16


class OceanFoamDepositSettings(ctypes.Structure):
    """ocean_foam_deposit_settings: one (generator, cascade) pair's deposit parameters, 8 bytes."""

    _fields_ = [
        ("amount", ctypes.c_float),
        ("per_speed", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanFoamDepositSettings) == 8


class OceanSpraySettings(ctypes.Structure):
    """ocean_spray_settings: one (generator, cascade) pair's emission parameters, 12 bytes."""

    _fields_ = [
        ("threshold", ctypes.c_float),
        ("rate", ctypes.c_float),
        ("seed", ctypes.c_uint32),
    ]


assert ctypes.sizeof(OceanSpraySettings) == 12


class OceanParticleSettings(ctypes.Structure):
    """ocean_particle_settings: one ocean_particles_step call's parameters, 40 bytes."""

    _fields_ = [
        ("gravity", ctypes.c_float),
        ("drag", ctypes.c_float),
        ("wind", ctypes.c_float * 3),
        ("lifetime", ctypes.c_float),
        ("gain", ctypes.c_float),
        ("lift", ctypes.c_float),
        ("iterations", ctypes.c_int32),
        ("tolerance", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanParticleSettings) == 40


class OceanHullStepSettings(ctypes.Structure):
    """ocean_hull_step_settings: one ocean_hulls_step call's parameters, 36 bytes."""

    _fields_ = [
        ("dt", ctypes.c_float),
        ("substeps", ctypes.c_int32),
        ("gravity", ctypes.c_float * 3),
        ("rho_g", ctypes.c_float),
        ("iterations", ctypes.c_int32),
        ("tolerance", ctypes.c_float),
        ("water_velocity", ctypes.c_int32),
    ]


assert ctypes.sizeof(OceanHullStepSettings) == 36


class OceanMooringSettings(ctypes.Structure):
    """ocean_mooring_settings: one ocean_moorings_step call's parameters, 48 bytes."""

    _fields_ = [
        ("dt", ctypes.c_float),
        ("substeps", ctypes.c_int32),
        ("gravity", ctypes.c_float * 3),
        ("rho_g", ctypes.c_float),
        ("iterations", ctypes.c_int32),
        ("tolerance", ctypes.c_float),
        ("water", ctypes.c_int32),
        ("bed_y", ctypes.c_float),
        ("bed_k", ctypes.c_float),
        ("bed_c", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanMooringSettings) == 48


class OceanWakeSettings(ctypes.Structure):
    """ocean_wake_settings: one ocean_wake_step call's parameters, 32 bytes."""

    _fields_ = [
        ("dt", ctypes.c_float),
        ("substeps", ctypes.c_int32),
        ("gravity", ctypes.c_float),
        ("rho_g", ctypes.c_float),
        ("damp", ctypes.c_float),
        ("edge_damp", ctypes.c_float),
        ("border", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


assert ctypes.sizeof(OceanWakeSettings) == 32


class OceanCamera(ctypes.Structure):
    """ocean_camera: position, world-space basis (viewInverse columns 0, 1 and -column 2), lens, 64 bytes."""

    _fields_ = [
        ("position", ctypes.c_float * 3),
        ("right", ctypes.c_float * 3),
        ("up", ctypes.c_float * 3),
        ("forward", ctypes.c_float * 3),
        ("tan_half_fov_y", ctypes.c_float),
        ("near_plane", ctypes.c_float),
        ("far_plane", ctypes.c_float),
        ("lod_scale", ctypes.c_float),
    ]


class OceanShading(ctypes.Structure):
    """ocean_shading: WaveRenderData of the reference's src/Renderer.h and the fog density, 76 bytes."""

    _fields_ = [
        ("wave_color", ctypes.c_float * 3),
        ("scatter_color", ctypes.c_float * 3),
        ("sky_color", ctypes.c_float * 3),
        ("light_color", ctypes.c_float * 3),
        ("light_direction", ctypes.c_float * 3),
        ("sun_view_angle", ctypes.c_float),
        ("sun_falloff_angle", ctypes.c_float),
        ("fog_begin", ctypes.c_float),
        ("fog_density", ctypes.c_float),
    ]


class OceanMarch(ctypes.Structure):
    """ocean_march: ocean_surface_raycast's parameters, 28 bytes."""

    _fields_ = [
        ("step", ctypes.c_float),
        ("max_steps", ctypes.c_int),
        ("refine", ctypes.c_int),
        ("iterations", ctypes.c_int),
        ("tolerance", ctypes.c_float),
        ("slope", ctypes.c_float),
        ("pad", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanCamera) == 64 and ctypes.sizeof(OceanShading) == 76 and ctypes.sizeof(OceanMarch) == 28


class OceanCameraLayers(ctypes.Structure):
    """ocean_camera_layers: the foam stage and the spray sprites of ocean_camera_render_layers, 48 bytes."""

    _fields_ = [
        ("foam_color", ctypes.c_float * 3),
        ("foam_lo", ctypes.c_float),
        ("foam_hi", ctypes.c_float),
        ("foam_opacity", ctypes.c_float),
        ("spray_color", ctypes.c_float * 3),
        ("spray_radius", ctypes.c_float),
        ("spray_max_half", ctypes.c_int32),
        ("spray_opacity", ctypes.c_float),
    ]


assert ctypes.sizeof(OceanCameraLayers) == 48

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_fp = ctypes.POINTER(ctypes.c_float)
_sp = ctypes.POINTER(OceanSettings)
_fsp = ctypes.POINTER(OceanFoamSettings)

# name -> (restype, argtypes); mirrors include/oceanfft.h one to one.
SIGNATURES = {
    "ocean_last_error": (ctypes.c_char_p, []),
    "ocean_version": (ctypes.c_char_p, []),
    "ocean_default_settings": (None, [_sp]),
    "ocean_device_count": (_i, []),
    "ocean_fft_create": (_i, [ctypes.POINTER(_vp), _sz, _vp]),
    "ocean_fft_destroy": (_i, [_vp]),
    "ocean_fft_texture_resolution": (_sz, [_vp]),
    "ocean_fft_encode_ifft": (_i, [_vp, _vp]),
    "ocean_fft_encode_ifft_batch": (_i, [_vp, _vp, _i]),
    "ocean_fft_synchronize": (_i, [_vp]),
    "ocean_fft_device_cus": (_i, [_vp]),
    "ocean_fft_set_cu_budget": (_i, [_vp, _i]),
    "ocean_generator_create": (_i, [ctypes.POINTER(_vp), _vp, _i]),
    "ocean_generator_destroy": (_i, [_vp]),
    "ocean_generator_cascades": (_i, [_vp]),
    "ocean_generator_settings": (_sp, [_vp, _i]),
    "ocean_generator_calculate": (_i, [_vp, _f, _i]),
    "ocean_generator_generate_spectrum": (_i, [_vp]),
    "ocean_generator_height_map": (_vp, [_vp, _i]),
    "ocean_generator_displacement_map": (_vp, [_vp, _i]),
    "ocean_generator_jacobian_map": (_vp, [_vp, _i]),
    "ocean_generator_initial_spectrum": (_vp, [_vp, _i]),
    "ocean_generator_spectrum_block": (_i, [_vp]),
    "ocean_generator_create_slab": (_i, [ctypes.POINTER(_vp), _vp, _i, _i]),
    "ocean_generator_exchange_bytes": (_sz, [_vp]),
    "ocean_generator_slab_columns": (_i, [_vp, _f, _i, _vp]),
    "ocean_generator_slab_rows": (_i, [_vp, _vp]),
    "ocean_generator_slab_info": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "ocean_generator_set_profiling": (_i, [_vp, _i]),
    "ocean_generator_kernel_times": (_i, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "ocean_debug_hash": (_i, [_vp, _i, _vp, _vp, _vp]),
    "ocean_debug_copy": (_i, [_vp, _vp, _sz, _i, _vp]),
    "ocean_debug_fft_work_limit": (_i, [_vp, _sz]),
    "ocean_surface_sample": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _vp]),
    "ocean_surface_sample_plane": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "ocean_surface_query": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _i, ctypes.c_float, _vp]),
    "ocean_generator_mip_levels": (_i, [_vp]),
    "ocean_generator_build_mips": (_i, [_vp]),
    "ocean_generator_height_mip": (_vp, [_vp, _i, _i]),
    "ocean_generator_displacement_mip": (_vp, [_vp, _i, _i]),
    "ocean_generator_jacobian_mip": (_vp, [_vp, _i, _i]),
    "ocean_surface_sample_lod": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _vp]),
    "ocean_surface_sample_plane_lod": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "ocean_generator_calculate_rates": (_i, [_vp]),
    "ocean_generator_height_rate_map": (_vp, [_vp, _i]),
    "ocean_generator_displacement_rate_map": (_vp, [_vp, _i]),
    "ocean_surface_velocity": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _vp]),
    "ocean_generator_set_depth_layers": (_i, [_vp, _fp, _i]),
    "ocean_generator_depth_layers": (_i, [_vp, _fp]),
    "ocean_generator_calculate_kinematics": (_i, [_vp]),
    "ocean_generator_kinematics_map": (_vp, [_vp, _i, _i, _i]),
    "ocean_water_kinematics": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _i, ctypes.c_float, _vp]),
    "ocean_generator_build_bounds": (_i, [_vp]),
    "ocean_generator_bounds": (_i, [_vp, _i, _fp]),
    "ocean_generator_bounds_device": (_vp, [_vp]),
    "ocean_surface_raycast": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _f, _i, _i, _i, _f, _f, _f, _vp]),
    "ocean_default_camera": (None, [ctypes.POINTER(OceanCamera)]),
    "ocean_default_shading": (None, [ctypes.POINTER(OceanShading)]),
    "ocean_default_march": (None, [ctypes.POINTER(OceanMarch)]),
    "ocean_camera_rays": (_i, [ctypes.POINTER(OceanCamera), _i, _i, _vp, _vp]),
    "ocean_camera_render": (_i, [_vp, _vp, _i, ctypes.POINTER(OceanCamera), ctypes.POINTER(OceanShading),
                                 ctypes.POINTER(OceanMarch), _i, _i, _vp, _vp, _vp]),
    "ocean_default_camera_layers": (None, [ctypes.POINTER(OceanCameraLayers)]),
    "ocean_camera_layers_scratch_bytes": (_sz, [_i, _i]),
    "ocean_camera_render_layers": (_i, [_vp, _vp, _i, ctypes.POINTER(OceanCamera), ctypes.POINTER(OceanShading),
                                        ctypes.POINTER(OceanMarch), ctypes.POINTER(OceanCameraLayers), _i, _i, _vp, _vp,
                                        ctypes.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "ocean_default_foam_settings": (None, [_fsp]),
    "ocean_generator_foam_settings": (_fsp, [_vp, _i]),
    "ocean_generator_advance_foam": (_i, [_vp, _f]),
    "ocean_generator_reset_foam": (_i, [_vp]),
    "ocean_generator_foam_map": (_vp, [_vp, _i]),
    "ocean_generator_foam_counts": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int64)]),
    "ocean_generator_foam_counts_device": (_vp, [_vp]),
    "ocean_surface_sample_foam": (_i, [_vp, _vp, _i, _vp, ctypes.c_int64, _vp]),
    "ocean_surface_sample_plane_foam": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "ocean_default_foam_deposit_settings": (None, [ctypes.POINTER(OceanFoamDepositSettings)]),
    "ocean_foam_deposit": (_i, [_vp, _vp, _i, ctypes.POINTER(OceanFoamDepositSettings), _vp, _vp, ctypes.c_int64]),
    "ocean_foam_deposit_counts": (_i, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "ocean_foam_deposit_counts_device": (_vp, [_vp]),
    "ocean_debug_foam_deposit_merge": (_i, [_i]),
    "ocean_hulls_create":(_i, [ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int64, _vp, _i]),
    "ocean_hulls_destroy": (_i, [_vp]),
    "ocean_hulls_bodies": (_i, [_vp]),
    "ocean_hulls_instance_points": (ctypes.c_int64, [_vp]),
    "ocean_debug_hulls_packing": (_i, [_i]),
    "ocean_hulls_loads": (_i, [_vp, _vp, _vp, _i, _vp, _f, _i, _f, _i, _vp, _vp]),
    "ocean_hulls_set_bodies": (_i, [_vp, _vp]),
    "ocean_default_hull_step_settings": (None, [ctypes.POINTER(OceanHullStepSettings)]),
    "ocean_hulls_step": (_i, [_vp, _vp, _vp, _i, ctypes.POINTER(OceanHullStepSettings), _vp, _vp, _vp, _vp]),
    "ocean_moorings_create": (_i, [ctypes.POINTER(_vp), _vp, _vp, _vp, _i, _i]),
    "ocean_moorings_destroy": (_i, [_vp]),
    "ocean_moorings_lines": (_i, [_vp]),
    "ocean_moorings_total_nodes": (ctypes.c_int64, [_vp]),
    "ocean_moorings_nodes": (_vp, [_vp]),
    "ocean_moorings_reset": (_i, [_vp, _vp]),
    "ocean_default_mooring_settings": (None, [ctypes.POINTER(OceanMooringSettings)]),
    "ocean_moorings_step": (_i, [_vp, _vp, _vp, _i, ctypes.POINTER(OceanMooringSettings), _vp, _vp, _vp]),
    "ocean_default_wake_settings": (None, [ctypes.POINTER(OceanWakeSettings)]),
    "ocean_wake_create": (_i, [ctypes.POINTER(_vp), _vp, _i, _f, _f, _f, _f]),
    "ocean_wake_destroy": (_i, [_vp]),
    "ocean_wake_size": (_i, [_vp]),
    "ocean_wake_kernel": (_i, [_vp, _fp]),
    "ocean_wake_max_substep": (ctypes.c_double, [_vp, _f]),
    "ocean_wake_origin": (_i, [_vp, _fp]),
    "ocean_wake_height": (_vp, [_vp]),
    "ocean_wake_reset": (_i, [_vp]),
    "ocean_wake_shift": (_i, [_vp, _i, _i]),
    "ocean_wake_step": (_i, [_vp, ctypes.POINTER(OceanWakeSettings), _vp, _vp, ctypes.c_int64]),
    "ocean_wake_sample": (_i, [_vp, _vp, ctypes.c_int64, _vp]),
    "ocean_debug_wake_create_host": (_i, [ctypes.POINTER(_vp), _i, _f, _f, _f, _f]),
    "ocean_default_spray_settings": (None, [ctypes.POINTER(OceanSpraySettings)]),
    "ocean_spray_create": (_i, [ctypes.POINTER(_vp), _vp]),
    "ocean_spray_destroy": (_i, [_vp]),
    "ocean_spray_emit": (_i, [_vp, _vp, _vp, _i, ctypes.POINTER(OceanSpraySettings), _vp, _f, ctypes.c_uint32, _i,
                              ctypes.c_int64, _vp]),
    "ocean_spray_counts": (_i, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "ocean_spray_counts_device": (_vp, [_vp]),
    "ocean_default_particle_settings": (None, [ctypes.POINTER(OceanParticleSettings)]),
    "ocean_particles_create": (_i, [ctypes.POINTER(_vp), _vp, ctypes.c_int64]),
    "ocean_particles_destroy": (_i, [_vp]),
    "ocean_particles_step": (_i, [_vp, _vp, _vp, _i, ctypes.POINTER(OceanParticleSettings), _f, _vp, _vp,
                                  ctypes.c_int64, _vp]),
    "ocean_particles_load": (_i, [_vp, _vp, ctypes.c_int64]),
    "ocean_particles_clear": (_i, [_vp]),
    "ocean_particles_records": (_vp, [_vp]),
    "ocean_particles_counts": (_i, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "ocean_particles_counts_device": (_vp, [_vp]),
    "ocean_generator_set_half_spectrum": (_i, [_vp, _i]),
    "ocean_generator_set_four_step": (_i, [_vp, _i]),
    "ocean_generator_set_h0_memo": (_i, [_vp, _i]),
    "ocean_generator_set_frame_overlap": (_i, [_vp, _i]),
    "ocean_generator_frame_bytes": (_i, [_vp, _vp]),
    "ocean_slab_layout": (_i, [_sz, _i, _i, _i, ctypes.POINTER(ctypes.c_int64)]),
    "ocean_comm_unique_id": (_i, [_vp]),
    "ocean_comm_create": (_i, [ctypes.POINTER(_vp), _vp, _i, _i]),
    "ocean_comm_wrap": (_i, [ctypes.POINTER(_vp), _vp, _i, _i]),
    "ocean_comm_destroy": (_i, [_vp]),
    "ocean_comm_all_to_all": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "ocean_generator_slab_frame": (_i, [_vp, _vp, _f, _i]),
    "ocean_generator_slab_frame_pipelined": (_i, [_vp, _vp, _f, _i]),
    "ocean_generator_slab_flush": (_i, [_vp]),
    "ocean_peers_create": (_i, [ctypes.POINTER(_vp), _vp]),
    "ocean_peers_destroy": (_i, [_vp]),
    "ocean_peers_handle": (_i, [_vp, _vp]),
    "ocean_peers_connect": (_i, [_vp, _vp]),
    "ocean_peers_connect_local": (_i, [ctypes.POINTER(_vp), _i]),
    "ocean_peers_set_timeout": (_i, [_vp, _i]),
    "ocean_peers_set_put_cus": (_i, [_vp, _i]),
    "ocean_peers_set_streams": (_i, [_vp, _vp, _vp, _vp]),
    "ocean_peers_set_row_cus": (_i, [_vp, _i]),
    "ocean_peers_set_put_cu_mask": (_i, [_vp, _i]),
    "ocean_generator_kernel_times4": (_i, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "ocean_generator_slab_frame_put": (_i, [_vp, _vp, _f, _i]),
    "ocean_generator_slab_frame_put_pipelined": (_i, [_vp, _vp, _f, _i]),
    "ocean_peers_flush": (_i, [_vp]),
    "ocean_frame_plan": (_i, [_sz, _i, ctypes.POINTER(ctypes.c_int32)]),
    "ocean_peers_debug_slot": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_sz)]),
    "ocean_generator_slab_put_columns": (_i, [_vp, _vp, _f, _i]),
    "ocean_generator_slab_put_rows": (_i, [_vp, _vp]),
    "ocean_peers_synchronize": (_i, [_vp]),
}

_lib = None


class OceanError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = lib().ocean_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with status {code}: {msg}")
        self.code = code


def lib():
    """Load liboceanfft.so (built in-tree by `make`); raises if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing — run `make` (or __graft_entry__.build()) first; "
                              "there is no CPU fallback for the ocean hot path")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code: int, where: str) -> None:
    if code != OCEAN_OK:
        raise OceanError(code, where)
