"""ctypes binding of libbhrt.so (the product: HIP kernels behind the C ABI of include/bhrt_api.h).

There is no CPU path here or in the library: if libbhrt.so is missing, or HIP is unusable,
calls raise BhrtError. Tests and the bench call the library through this module.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEFAULT_PATH = os.path.join(_PKG_DIR, "libbhrt.so")
LIB_PATH = os.environ.get("BHRT_LIB", _DEFAULT_PATH)


class BhrtError(RuntimeError):
    pass


_lib = None

# exported symbols and their prototypes (restype, argtypes)
_P = C.POINTER
_PROTOS = {
    "trace_ray": (C.c_int, [_P(abi.Ray), _P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                            _P(abi.SimulationConfig), _P(abi.RayTraceHit)]),
    "trace_rays_batch": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                   _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                   C.c_void_p, C.c_int]),
    "integrate_photon_path": (C.c_int, [_P(abi.Vector4D), _P(abi.Vector3D),
                                        _P(abi.BlackHoleParams), _P(abi.SimulationConfig), C.c_int,
                                        C.c_void_p, C.c_int, _P(C.c_int), _P(abi.RayTraceHit)]),
    "trace_pixel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P(abi.Vector3D),
                              _P(abi.Vector3D), _P(abi.Vector3D), C.c_double,
                              _P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                              _P(abi.SimulationConfig), _P(abi.SupersamplingParams),
                              _P(abi.AdaptiveSamplingParams), _P(C.c_double * 3)]),
    "bhrt_render_frame": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                    _P(abi.SimulationConfig), _P(abi.Camera), C.c_int, C.c_int,
                                    C.c_int, C.c_int, _P(abi.FrameSoA)]),
    "bhrt_render_frame_async": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                          _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                          C.c_int, C.c_int, C.c_int, _P(abi.FrameSoA),
                                          _P(C.c_int)]),
    "bhrt_frame_wait": (C.c_int, [C.c_int]),
    "bhrt_render_frame_device": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                           _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                           C.c_int, _P(abi.Rows), C.c_int, C.c_int,
                                           _P(abi.FrameSoA), C.c_void_p]),
    "bhrt_render_frame_gather": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                           _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                           C.c_int, C.c_int, C.c_int, _P(abi.FrameSoA), C.c_int,
                                           C.c_int, C.c_void_p]),
    "bhrt_sample_offsets": (C.c_int, [_P(abi.SupersamplingParams),
                                      _P(abi.AdaptiveSamplingParams), C.c_void_p, C.c_void_p,
                                      C.c_int]),
    "bhrt_render_frame_ss_device": (C.c_int, [_P(abi.BlackHoleParams),
                                              _P(abi.AccretionDiskParams),
                                              _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                              C.c_int, _P(abi.Rows), C.c_int, C.c_int,
                                              _P(abi.SupersamplingParams),
                                              _P(abi.AdaptiveSamplingParams), _P(abi.FrameSoA),
                                              C.c_void_p]),
    "bhrt_render_frame_ss": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                       _P(abi.SimulationConfig), _P(abi.Camera), C.c_int, C.c_int,
                                       C.c_int, C.c_int, _P(abi.SupersamplingParams),
                                       _P(abi.AdaptiveSamplingParams), _P(abi.FrameSoA)]),
    "bhrt_render_frame_adaptive_device": (C.c_int, [_P(abi.BlackHoleParams),
                                                    _P(abi.AccretionDiskParams),
                                                    _P(abi.SimulationConfig), _P(abi.Camera),
                                                    C.c_int, C.c_int, _P(abi.Rows), C.c_int,
                                                    C.c_int, _P(abi.SupersamplingParams),
                                                    _P(abi.AdaptiveSamplingParams),
                                                    _P(abi.FrameSoA), C.c_void_p,
                                                    _P(abi.AdaptiveInfo), C.c_void_p]),
    "bhrt_render_frame_adaptive": (C.c_int, [_P(abi.BlackHoleParams),
                                             _P(abi.AccretionDiskParams),
                                             _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                             C.c_int, C.c_int, C.c_int,
                                             _P(abi.SupersamplingParams),
                                             _P(abi.AdaptiveSamplingParams), _P(abi.FrameSoA),
                                             C.c_void_p, _P(abi.AdaptiveInfo)]),
    "bhrt_accum_alpha": (C.c_float, [_P(abi.AccumParams), C.c_int]),
    "bhrt_accum_create": (C.c_int, [C.c_int, C.c_int, _P(abi.Rows), _P(abi.AccumParams),
                                    _P(C.c_void_p)]),
    "bhrt_accum_destroy": (None, [C.c_void_p]),
    "bhrt_accum_reset": (C.c_int, [C.c_void_p]),
    "bhrt_accum_info": (C.c_int, [C.c_void_p, _P(abi.SupersamplingParams), _P(abi.AccumState)]),
    "bhrt_accum_device_buffers": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "bhrt_accum_frame_device": (C.c_int, [C.c_void_p, _P(abi.BlackHoleParams),
                                          _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                          _P(abi.Camera), C.c_int, C.c_int,
                                          _P(abi.SupersamplingParams), _P(abi.AccumOut),
                                          C.c_void_p]),
    "bhrt_accum_blend_device": (C.c_int, [C.c_void_p, C.c_void_p, _P(abi.AccumOut), C.c_void_p]),
    "bhrt_accum_frame": (C.c_int, [C.c_void_p, _P(abi.BlackHoleParams),
                                   _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                   _P(abi.Camera), C.c_int, C.c_int, _P(abi.SupersamplingParams),
                                   _P(abi.AccumOut)]),
    "bhrt_particles_create": (C.c_int, [_P(abi.ParticleSystem), _P(C.c_void_p)]),
    "bhrt_particles_upload": (C.c_int, [C.c_void_p, _P(abi.ParticleSystem)]),
    "bhrt_particles_update_device": (C.c_int, [C.c_void_p, _P(abi.BlackHoleParams),
                                               _P(abi.SimulationConfig), C.c_int, C.c_void_p]),
    "bhrt_particles_extract_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.ParticleData),
                                                C.c_void_p]),
    "bhrt_particles_extract": (C.c_int, [C.c_void_p, C.c_int, _P(abi.ParticleData)]),
    "bhrt_particles_download": (C.c_int, [C.c_void_p, _P(abi.ParticleSystem)]),
    "bhrt_particles_device_buffer": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int)]),
    "bhrt_particles_info": (C.c_int, [C.c_void_p, _P(abi.ParticlesState)]),
    "bhrt_particles_destroy": (None, [C.c_void_p]),
    "bhrt_particles_kernel_ms": (C.c_int, [C.c_void_p, _P(abi.BlackHoleParams),
                                           _P(abi.SimulationConfig), C.c_int,
                                           _P(abi.ParticleData), _P(C.c_double * 5)]),
    "bhrt_sky_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_void_p)]),
    "bhrt_sky_destroy": (None, [C.c_void_p]),
    "bhrt_sky_info": (C.c_int, [C.c_void_p, _P(abi.SkyState)]),
    "bhrt_set_sky": (C.c_int, [C.c_void_p]),
    "bhrt_sky_lookup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "bhrt_sky_lookup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bhrt_kerr_frame_device": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                         _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                         C.c_int, _P(abi.Rows), C.c_int, _P(abi.FrameSoA),
                                         _P(abi.KerrDiag), C.c_void_p]),
    "bhrt_kerr_frame": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                  _P(abi.SimulationConfig), _P(abi.Camera), C.c_int, C.c_int,
                                  C.c_int, _P(abi.FrameSoA), _P(abi.KerrDiag)]),
    "bhrt_kerr_rays_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                        _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                        C.c_int, _P(abi.FrameSoA), _P(abi.KerrDiag), C.c_void_p]),
    "bhrt_kerr_rays": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                 _P(abi.AccretionDiskParams), _P(abi.SimulationConfig), C.c_int,
                                 _P(abi.FrameSoA), _P(abi.KerrDiag)]),
    "bhrt_kerr_rk45_frame_device": (C.c_int, [_P(abi.BlackHoleParams),
                                              _P(abi.AccretionDiskParams),
                                              _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                              C.c_int, _P(abi.Rows), C.c_int, _P(abi.FrameSoA),
                                              _P(abi.KerrRk45Diag), C.c_void_p]),
    "bhrt_kerr_rk45_frame": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                       _P(abi.SimulationConfig), _P(abi.Camera), C.c_int, C.c_int,
                                       C.c_int, _P(abi.FrameSoA), _P(abi.KerrRk45Diag)]),
    "bhrt_kerr_rk45_rays_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                             _P(abi.AccretionDiskParams),
                                             _P(abi.SimulationConfig), C.c_int, _P(abi.FrameSoA),
                                             _P(abi.KerrRk45Diag), C.c_void_p]),
    "bhrt_kerr_rk45_rays": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                      _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                      C.c_int, _P(abi.FrameSoA), _P(abi.KerrRk45Diag)]),
    "bhrt_kerr_emit_frame_device": (C.c_int, [_P(abi.BlackHoleParams),
                                              _P(abi.AccretionDiskParams),
                                              _P(abi.SimulationConfig), _P(abi.Camera), C.c_int,
                                              C.c_int, _P(abi.Rows), C.c_int, _P(abi.FrameSoA),
                                              _P(abi.KerrRk45Diag), _P(abi.KerrEmitParams),
                                              _P(abi.KerrEmitOut), C.c_void_p]),
    "bhrt_kerr_emit_frame": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.AccretionDiskParams),
                                       _P(abi.SimulationConfig), _P(abi.Camera), C.c_int, C.c_int,
                                       C.c_int, _P(abi.FrameSoA), _P(abi.KerrRk45Diag),
                                       _P(abi.KerrEmitParams), _P(abi.KerrEmitOut)]),
    "bhrt_kerr_emit_rays_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                             _P(abi.AccretionDiskParams),
                                             _P(abi.SimulationConfig), C.c_int, _P(abi.FrameSoA),
                                             _P(abi.KerrRk45Diag), _P(abi.KerrEmitParams),
                                             _P(abi.KerrEmitOut), C.c_void_p]),
    "bhrt_kerr_emit_rays": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                      _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                      C.c_int, _P(abi.FrameSoA), _P(abi.KerrRk45Diag),
                                      _P(abi.KerrEmitParams), _P(abi.KerrEmitOut)]),
    "bhrt_kerr_disk_redshift": (C.c_int, [_P(abi.BlackHoleParams), C.c_double, C.c_double,
                                          C.c_double, _P(C.c_double)]),
    "bhrt_kerr_paths_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                         _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                         C.c_int, C.c_int, C.c_int, _P(abi.Paths),
                                         _P(abi.FrameSoA), _P(abi.KerrDiag), C.c_void_p]),
    "bhrt_kerr_paths": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                  _P(abi.AccretionDiskParams), _P(abi.SimulationConfig), C.c_int,
                                  C.c_int, C.c_int, _P(abi.Paths), _P(abi.FrameSoA),
                                  _P(abi.KerrDiag)]),
    "bhrt_kerr_ray_init": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.Vector3D), _P(abi.Vector3D),
                                     _P(C.c_double * 6), _P(C.c_double)]),
    "bhrt_particles_kerr_update_device": (C.c_int, [C.c_void_p, _P(abi.BlackHoleParams),
                                                    _P(abi.SimulationConfig), C.c_int,
                                                    _P(abi.KerrParticlesParams),
                                                    _P(abi.KerrParticlesDiag), C.c_void_p]),
    "bhrt_kerr_particle_state": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.Vector3D),
                                           _P(abi.Vector3D), _P(C.c_double * 6), _P(C.c_double),
                                           _P(C.c_double)]),
    "bhrt_kerr_orbit_velocity": (C.c_int, [_P(abi.BlackHoleParams), _P(abi.Vector3D), C.c_int,
                                           _P(abi.Vector3D)]),
    "bhrt_trace_rays": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                  _P(abi.AccretionDiskParams), _P(abi.SimulationConfig), C.c_int,
                                  C.c_int, _P(abi.FrameSoA)]),
    "bhrt_trace_rays_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                         _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                         C.c_int, C.c_int, _P(abi.FrameSoA), C.c_void_p]),
    "bhrt_trace_paths_device": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                          _P(abi.AccretionDiskParams), _P(abi.SimulationConfig),
                                          C.c_int, C.c_int, C.c_int, _P(abi.Paths),
                                          _P(abi.FrameSoA), C.c_void_p]),
    "bhrt_trace_paths": (C.c_int, [C.c_void_p, C.c_int, _P(abi.BlackHoleParams),
                                   _P(abi.AccretionDiskParams), _P(abi.SimulationConfig), C.c_int,
                                   C.c_int, C.c_int, _P(abi.Paths), _P(abi.FrameSoA)]),
    "bhrt_check_guard_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "bhrt_shard_rows": (C.c_int, [C.c_int, _P(abi.Rows)]),
    "bhrt_get_stats": (C.c_int, [_P(abi.Stats), C.c_int]),
    "bhrt_device_count": (C.c_int, []),
    "bhrt_set_refill_threshold": (None, [C.c_int]),
    "bhrt_set_claim_order": (C.c_int, [C.c_void_p, C.c_int]),
    "bhrt_last_error": (C.c_char_p, []),
    "bh_initialize": (C.c_void_p, []),
    "bh_shutdown": (None, [C.c_void_p]),
    "bh_configure_black_hole": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "bh_configure_accretion_disk": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double,
                                              C.c_double]),
    "bh_configure_simulation": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int,
                                          C.c_double]),
    "bh_trace_ray": (C.c_int, [C.c_void_p, _P(C.c_double * 3), _P(C.c_double * 3),
                               _P(abi.RayTraceHit)]),
    "bh_trace_rays_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "bh_get_version": (None, [_P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "bh_calculate_time_dilation": (C.c_int, [C.c_void_p, _P(C.c_double * 3),
                                             _P(C.c_double * 3), _P(C.c_double)]),
    "calculate_disk_temperature": (None, [_P(abi.Vector3D), _P(abi.BlackHoleParams),
                                          _P(abi.AccretionDiskParams), _P(C.c_double),
                                          _P(C.c_double * 3)]),
    "apply_relativistic_effects": (None, [_P(abi.Vector3D), _P(abi.Vector3D),
                                          _P(abi.BlackHoleParams), _P(C.c_double * 3),
                                          _P(C.c_double)]),
    "temperature_to_rgb": (None, [C.c_double, _P(C.c_double * 3)]),
    "halton_sequence": (C.c_double, [C.c_int, C.c_int]),
    "get_isco_radius": (C.c_double, [_P(abi.BlackHoleParams)]),
    "initialize_black_hole_params": (None, [_P(abi.BlackHoleParams), C.c_double, C.c_double,
                                            C.c_double]),
    "check_disk_intersection": (C.c_int, [_P(abi.Vector3D), _P(abi.Vector3D), _P(abi.Vector3D),
                                          _P(abi.AccretionDiskParams), _P(abi.Vector3D)]),
}


def _one_hip_runtime():
    """Import torch (if installed) before libbhrt is mapped. The torch wheel carries its own HIP
    runtime, torch/lib/libamdhip64.so, whose SONAME is libamdhip64.so.7 -- the name libbhrt.so
    needs. Loaded first, it is the process's one runtime and libbhrt binds to it (torch's device
    buffers and streams are then libbhrt's too). Loaded after libbhrt, torch -- which needs the
    library by its file name -- maps a second runtime next to /opt/rocm's, and its device
    initialisation fails ("No HIP GPUs are available", tools/torch_after_lib.py).
    BHRT_PY_NO_TORCH=1 skips it (a torch-free process then runs /opt/rocm's runtime)."""
    if os.environ.get("BHRT_PY_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    except Exception as e:  # a broken torch (its bundled HIP runtime failed to load): go on
        import warnings     # with /opt/rocm's runtime, which libbhrt finds by its SONAME
        warnings.warn(f"torch failed to import ({e!r}); libbhrt binds /opt/rocm's HIP runtime")


def load(path=None):
    """Load libbhrt.so once; raise BhrtError (never fall back) if it is not there."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise BhrtError(f"libbhrt.so not built at {p} (run __graft_entry__.build())")
    _one_hip_runtime()
    lib = C.CDLL(p)
    older = p != _DEFAULT_PATH  # an A/B build of an earlier revision may lack newer entry points
    for name, (res, args) in _PROTOS.items():
        if older and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(x):
    return C.byref(x) if x is not None else None


def last_error():
    return (load().bhrt_last_error() or b"").decode()


def _check(rc, what):
    if rc != 0:
        raise BhrtError(f"{what} failed: {last_error()}")


def render_frame(bh, dk, cfg, cam, width, height, method=abi.INTEGRATOR_RK4, flags=0,
                 fields=abi.SOA_FIELDS):
    """bhrt_render_frame into host numpy arrays (all visible GPUs)."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    _check(load().bhrt_render_frame(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height,
                                    method, flags, C.byref(soa)), "bhrt_render_frame")
    return arrays


def trace_rays(rays, bh, dk, cfg, method=abi.INTEGRATOR_RK4, flags=0, fields=abi.SOA_FIELDS):
    """bhrt_trace_rays: rays is a numpy array of abi.RAY_DTYPE."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    arrays, soa = abi.alloc_soa(len(rays), fields)
    _check(load().bhrt_trace_rays(rays.ctypes.data, len(rays), _ptr(bh), _ptr(dk), _ptr(cfg),
                                  method, flags, C.byref(soa)), "bhrt_trace_rays")
    return arrays


def trace_rays_batch(rays, bh, dk, cfg):
    """The drop-in trace_rays_batch; returns (rc, hits as abi.HIT_DTYPE array)."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    hits = np.zeros(len(rays), dtype=abi.HIT_DTYPE)
    rc = load().trace_rays_batch(rays.ctypes.data, len(rays), _ptr(bh), _ptr(dk), _ptr(cfg),
                                 hits.ctypes.data, 0)
    return rc, hits


def soa_from_tensors(tensors):
    """FrameSoA pointing at device tensors (torch), keyed by abi.SOA_FIELDS names."""
    return abi.FrameSoA(**{f: t.data_ptr() for f, t in tensors.items()})


def render_frame_device(bh, dk, cfg, cam, width, height, rows, method, flags, soa, stream):
    """Asynchronous launch into device SoA buffers on a hipStream_t (int handle or None)."""
    _check(load().bhrt_render_frame_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                           height, _ptr(rows), method, flags, C.byref(soa),
                                           C.c_void_p(stream) if stream else None),
           "bhrt_render_frame_device")


def render_frame_gather(bh, dk, cfg, cam, width, height, method, flags, soa, ndev=0, shards=0,
                        stream=None):
    """bhrt_render_frame_gather: the frame rendered by ndev devices in `shards` cyclic shards and
    gathered into root-device SoA buffers (the current device) on a hipStream_t."""
    _check(load().bhrt_render_frame_gather(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                           height, method, flags, C.byref(soa), int(ndev),
                                           int(shards),
                                           C.c_void_p(stream) if stream else None),
           "bhrt_render_frame_gather")


SS_MAX_SAMPLES = 64  # BHRT_SS_MAX_SAMPLES
SS_FIELDS = ("result", "rgb_r", "rgb_g", "rgb_b", "rgba32f", "rgba8")


def sample_offsets(ss, as_=None):
    """bhrt_sample_offsets: trace_pixel's sub-pixel offsets for these SupersamplingParams /
    AdaptiveSamplingParams (either may be None), as a float64 array [count, 2]."""
    ox = np.zeros(SS_MAX_SAMPLES)
    oy = np.zeros(SS_MAX_SAMPLES)
    n = load().bhrt_sample_offsets(_ptr(ss), _ptr(as_), ox.ctypes.data, oy.ctypes.data,
                                   SS_MAX_SAMPLES)
    if n < 0:
        raise BhrtError(f"bhrt_sample_offsets failed: {last_error()}")
    return np.stack([ox[:n], oy[:n]], axis=1)


def render_frame_ss_device(bh, dk, cfg, cam, width, height, rows, method, flags, ss, as_, soa,
                           stream):
    """bhrt_render_frame_ss_device: (a shard of) a frame of trace_pixel sample averages into
    device SoA buffers (result, rgb_*, rgba32f, rgba8), asynchronous on a hipStream_t (int handle
    or None)."""
    _check(load().bhrt_render_frame_ss_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                              height, _ptr(rows), method, flags, _ptr(ss),
                                              _ptr(as_), C.byref(soa),
                                              C.c_void_p(stream) if stream else None),
           "bhrt_render_frame_ss_device")


def render_frame_ss(bh, dk, cfg, cam, width, height, method=abi.INTEGRATOR_RK4, flags=0, ss=None,
                    as_=None, fields=SS_FIELDS):
    """bhrt_render_frame_ss into host numpy arrays (the current device)."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    _check(load().bhrt_render_frame_ss(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height,
                                       method, flags, _ptr(ss), _ptr(as_), C.byref(soa)),
           "bhrt_render_frame_ss")
    return arrays


def _info_dict(info):
    return {f: int(getattr(info, f)) for f, _ in abi.AdaptiveInfo._fields_}


def render_frame_adaptive_device(bh, dk, cfg, cam, width, height, rows, method, flags, ss, as_,
                                 soa, samples_ptr, stream):
    """bhrt_render_frame_adaptive_device: (a shard of) a frame with as_.min_samples samples per
    pixel and as_.max_samples at the edge pixels (the rule: include/bhrt_api.h) into device SoA
    buffers and, if samples_ptr is not None, the int32 device array of S(p); on a hipStream_t
    (int handle or None). Returns the call's bhrt_adaptive_info as a dict."""
    info = abi.AdaptiveInfo()
    _check(load().bhrt_render_frame_adaptive_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam),
                                                    width, height, _ptr(rows), method, flags,
                                                    _ptr(ss), _ptr(as_), C.byref(soa),
                                                    samples_ptr, C.byref(info),
                                                    C.c_void_p(stream) if stream else None),
           "bhrt_render_frame_adaptive_device")
    return _info_dict(info)


def render_frame_adaptive(bh, dk, cfg, cam, width, height, method=abi.INTEGRATOR_RK4, flags=0,
                          ss=None, as_=None, fields=SS_FIELDS):
    """bhrt_render_frame_adaptive into host numpy arrays (the current device): the fields, plus
    `samples` (S(p), int32) and `info` (the call's bhrt_adaptive_info as a dict)."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    samples = np.zeros(width * height, dtype=np.int32)
    info = abi.AdaptiveInfo()
    _check(load().bhrt_render_frame_adaptive(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                             height, method, flags, _ptr(ss), _ptr(as_),
                                             C.byref(soa), samples.ctypes.data, C.byref(info)),
           "bhrt_render_frame_adaptive")
    arrays["samples"] = samples
    arrays["info"] = _info_dict(info)
    return arrays


def accum_alpha(params, frame_count):
    """bhrt_accum_alpha: the blend weight of the step at this frame_count (params None: the
    defaults), as the float32 the library uses."""
    return np.float32(load().bhrt_accum_alpha(_ptr(params), int(frame_count)))


def accum_create(width, height, rows=None, params=None):
    """bhrt_accum_create on the current device: the handle (an int) for the accum_* calls; free
    it with accum_destroy."""
    h = C.c_void_p()
    _check(load().bhrt_accum_create(int(width), int(height), _ptr(rows), _ptr(params),
                                    C.byref(h)), "bhrt_accum_create")
    return h.value


def accum_destroy(acc):
    load().bhrt_accum_destroy(acc)


def accum_reset(acc):
    """bhrt_accum_reset: the next step starts from an empty image."""
    _check(load().bhrt_accum_reset(acc), "bhrt_accum_reset")


def accum_state(acc, ss=None):
    """bhrt_accum_info: the host-side state as a dict (cycle and the next offset for `ss`)."""
    s = abi.AccumState()
    _check(load().bhrt_accum_info(acc, _ptr(ss), C.byref(s)), "bhrt_accum_info")
    return {f: getattr(s, f) for f, _ in abi.AccumState._fields_}


def accum_device_buffers(acc):
    """bhrt_accum_device_buffers: (acc [n][3] float32, edge [n] float32) device addresses."""
    rgb, edge = C.c_void_p(), C.c_void_p()
    _check(load().bhrt_accum_device_buffers(acc, C.byref(rgb), C.byref(edge)),
           "bhrt_accum_device_buffers")
    return rgb.value, edge.value


def accum_out(tensors):
    """abi.AccumOut pointing at device tensors (torch) keyed rgba8 / rgb / edge_factor."""
    return abi.AccumOut(**{f: t.data_ptr() for f, t in tensors.items()})


def accum_frame_device(acc, bh, dk, cfg, cam, method, flags, ss, out, stream):
    """bhrt_accum_frame_device: one rendered step of the accumulator -- the plain frame at the
    next offset of `ss`, blended, with the display bytes and edge factors -- into the device
    buffers of `out` (abi.AccumOut), asynchronous on a hipStream_t (int handle or None)."""
    _check(load().bhrt_accum_frame_device(acc, _ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), method,
                                          flags, _ptr(ss), _ptr(out),
                                          C.c_void_p(stream) if stream else None),
           "bhrt_accum_frame_device")


def accum_blend_device(acc, rgb_ptr, out, stream):
    """bhrt_accum_blend_device: one step with the caller's device frame ([n][3] float32 at
    rgb_ptr); `out` may be None."""
    _check(load().bhrt_accum_blend_device(acc, rgb_ptr, _ptr(out),
                                          C.c_void_p(stream) if stream else None),
           "bhrt_accum_blend_device")


def accum_frame(acc, bh, dk, cfg, cam, method=abi.INTEGRATOR_RK4, flags=0, ss=None,
                fields=("rgba8", "rgb", "edge_factor")):
    """bhrt_accum_frame: one rendered step into host numpy arrays (a dict of `fields`)."""
    n = accum_state(acc)["pixels"]
    shape = {"rgba8": ((n, 4), np.uint8), "rgb": ((n, 3), np.float32),
             "edge_factor": ((n,), np.float32)}
    arrays = {f: np.zeros(*shape[f]) for f in fields}
    out = abi.AccumOut(**{f: a.ctypes.data for f, a in arrays.items()})
    _check(load().bhrt_accum_frame(acc, _ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), method, flags,
                                   _ptr(ss), C.byref(out)), "bhrt_accum_frame")
    return arrays


def particles_create(system):
    """bhrt_particles_create on the current device: a resident copy of the abi.ParticleSystem's
    particles; the handle (an int) for the particles_* calls, freed with particles_destroy."""
    h = C.c_void_p()
    _check(load().bhrt_particles_create(_ptr(system), C.byref(h)), "bhrt_particles_create")
    return h.value


def particles_destroy(ps):
    load().bhrt_particles_destroy(ps)


def particles_upload(ps, system):
    """bhrt_particles_upload: the host system's array again (its count may have changed)."""
    _check(load().bhrt_particles_upload(ps, _ptr(system)), "bhrt_particles_upload")


def particles_update_device(ps, bh, cfg, steps=1, stream=None):
    """bhrt_particles_update_device: `steps` update_particles steps of the resident array,
    asynchronous on a hipStream_t (int handle or None)."""
    _check(load().bhrt_particles_update_device(ps, _ptr(bh), _ptr(cfg), int(steps),
                                               C.c_void_p(stream) if stream else None),
           "bhrt_particles_update_device")


def particle_data(tensors):
    """abi.ParticleData pointing at device tensors (torch) keyed by abi.PARTICLE_DATA_FIELDS."""
    return abi.ParticleData(**{f: t.data_ptr() for f, t in tensors.items()})


def particles_extract_device(ps, max_count, out, stream=None):
    """bhrt_particles_extract_device: bh_get_particle_data of the resident array into the device
    arrays of `out` (abi.ParticleData), asynchronous on a hipStream_t (int handle or None)."""
    _check(load().bhrt_particles_extract_device(ps, int(max_count), _ptr(out),
                                                C.c_void_p(stream) if stream else None),
           "bhrt_particles_extract_device")


def particles_extract(ps, max_count, fields=abi.PARTICLE_DATA_FIELDS, fill=0):
    """bhrt_particles_extract into host numpy arrays of max_count elements (a dict of `fields`;
    elements at and beyond count[0] keep `fill`)."""
    arrays = {}
    for f in fields:
        if f == "count":
            arrays[f] = np.full(1, fill, dtype=np.int32)
        else:
            tail, dtype = abi.PARTICLE_DATA_SHAPES[f]
            arrays[f] = np.full((int(max_count),) + tail, fill, dtype=dtype)
    out = abi.ParticleData(**{f: a.ctypes.data for f, a in arrays.items()})
    _check(load().bhrt_particles_extract(ps, int(max_count), C.byref(out)),
           "bhrt_particles_extract")
    return arrays


def particles_download(ps, system):
    """bhrt_particles_download: the resident particles into system.particles (equal counts)."""
    _check(load().bhrt_particles_download(ps, _ptr(system)), "bhrt_particles_download")


def particles_device_buffer(ps):
    """bhrt_particles_device_buffer: (device address of the Particle array, count)."""
    p, n = C.c_void_p(), C.c_int()
    _check(load().bhrt_particles_device_buffer(ps, C.byref(p), C.byref(n)),
           "bhrt_particles_device_buffer")
    return p.value, n.value


def particles_state(ps):
    """bhrt_particles_info: the host-side state as a dict (count, device, updates)."""
    s = abi.ParticlesState()
    _check(load().bhrt_particles_info(ps, C.byref(s)), "bhrt_particles_info")
    return {f: getattr(s, f) for f, _ in abi.ParticlesState._fields_}


def particles_kernel_ms(ps, bh, cfg, max_count, out):
    """bhrt_particles_kernel_ms: HIP-event times (ms) of a plain update, a counting update (each
    the second of two), the scan, the scatter into the device arrays of `out` and the count pass;
    the resident array advances four steps."""
    ms = (C.c_double * 5)()
    _check(load().bhrt_particles_kernel_ms(ps, _ptr(bh), _ptr(cfg), int(max_count), _ptr(out),
                                           C.byref(ms)), "bhrt_particles_kernel_ms")
    return dict(zip(("update_plain", "update_counted", "scan", "scatter", "count_pass"), ms))


def sky_create(texels):
    """bhrt_sky_create on the current device from a numpy map: float32 [H, W, 3]
    (BHRT_SKY_RGB32F) or uint8 [H, W, 4] (BHRT_SKY_RGBA8). The handle (an int) for the sky_*
    calls and set_sky; free it with sky_destroy."""
    t = np.ascontiguousarray(texels)
    if t.dtype == np.uint8 and t.ndim == 3 and t.shape[2] == 4:
        fmt = abi.BHRT_SKY_RGBA8
    elif t.dtype == np.float32 and t.ndim == 3 and t.shape[2] == 3:
        fmt = abi.BHRT_SKY_RGB32F
    else:
        raise BhrtError("sky_create: texels must be float32 [H, W, 3] or uint8 [H, W, 4]")
    h = C.c_void_p()
    _check(load().bhrt_sky_create(t.ctypes.data, t.shape[1], t.shape[0], fmt, C.byref(h)),
           "bhrt_sky_create")
    return h.value


def sky_destroy(sky):
    load().bhrt_sky_destroy(sky)


def sky_state(sky):
    """bhrt_sky_info as a dict (width, height, format, device)."""
    s = abi.SkyState()
    _check(load().bhrt_sky_info(sky, C.byref(s)), "bhrt_sky_info")
    return {f: getattr(s, f) for f, _ in abi.SkyState._fields_}


def set_sky(sky):
    """bhrt_set_sky: the calling thread's map for frames with abi.BHRT_FLAG_SKY; None unbinds."""
    _check(load().bhrt_set_sky(sky), "bhrt_set_sky")


def sky_lookup_device(sky, dirs_ptr, n, rgb_ptr, stream=None):
    """bhrt_sky_lookup_device: the lookup of n packed device vectors ([n][3] float64) into
    [n][3] float64 device colours, asynchronous on a hipStream_t (int handle or None)."""
    _check(load().bhrt_sky_lookup_device(sky, dirs_ptr, int(n), rgb_ptr,
                                         C.c_void_p(stream) if stream else None),
           "bhrt_sky_lookup_device")


def sky_lookup(sky, dirs):
    """bhrt_sky_lookup: the lookup of host vectors [n, 3]; returns float64 [n, 3]."""
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    rgb = np.zeros_like(d)
    _check(load().bhrt_sky_lookup(sky, d.ctypes.data, len(d), rgb.ctypes.data), "bhrt_sky_lookup")
    return rgb


def trace_paths_device(rays_ptr, n, bh, dk, cfg, method, max_positions, every, paths, hits,
                       stream):
    """bhrt_trace_paths_device: the recorded paths of n device rays (AoS Ray[n] at rays_ptr) into
    the device arrays of `paths` (abi.Paths) and, if not None, the hit fields of `hits`
    (abi.FrameSoA), asynchronous on a hipStream_t (int handle or None)."""
    _check(load().bhrt_trace_paths_device(rays_ptr, int(n), _ptr(bh), _ptr(dk), _ptr(cfg), method,
                                          int(max_positions), int(every), _ptr(paths),
                                          _ptr(hits), C.c_void_p(stream) if stream else None),
           "bhrt_trace_paths_device")


def trace_paths(rays, bh, dk, cfg, method=abi.INTEGRATOR_RK4, max_positions=1001, every=1,
                f32=False, fill=np.nan):
    """bhrt_trace_paths into host numpy arrays: rays is a numpy array of abi.RAY_DTYPE. Returns a
    dict with `xyz` [n, max_positions, 3] (float32 with f32, else float64; elements beyond a
    ray's count keep `fill`), `count` [n] and the hit fields (abi.PATH_HIT_FIELDS)."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    n = len(rays)
    xyz = np.full((n, int(max_positions), 3), fill, dtype=np.float32 if f32 else np.float64)
    count = np.zeros(n, dtype=np.int32)
    paths = abi.Paths(xyz=None if f32 else xyz.ctypes.data, xyz32=xyz.ctypes.data if f32 else None,
                      count=count.ctypes.data)
    arrays, soa = abi.alloc_soa(n, abi.PATH_HIT_FIELDS)
    _check(load().bhrt_trace_paths(rays.ctypes.data, n, _ptr(bh), _ptr(dk), _ptr(cfg), method,
                                   int(max_positions), int(every), C.byref(paths), C.byref(soa)),
           "bhrt_trace_paths")
    arrays["xyz"] = xyz
    arrays["count"] = count
    return arrays


KERR_FIELDS = tuple(f for f in abi.SOA_FIELDS if f != "time_dilation")  # never produced here


def _kerr_host_diag(n, diag):
    if not diag:
        return {}, None
    arrays = {"h_residual": np.zeros(n), "lz_drift": np.zeros(n)}
    return arrays, abi.KerrDiag(arrays["h_residual"].ctypes.data, arrays["lz_drift"].ctypes.data)


def kerr_frame_device(bh, dk, cfg, cam, width, height, rows, flags, soa, diag=None, stream=None):
    """bhrt_kerr_frame_device: (a shard of) a camera frame of physical Kerr geodesics into device
    SoA buffers, asynchronous on a hipStream_t (int handle or None); diag an abi.KerrDiag of
    device pointers or None."""
    _check(load().bhrt_kerr_frame_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height,
                                         _ptr(rows), flags, C.byref(soa), _ptr(diag),
                                         C.c_void_p(stream) if stream else None),
           "bhrt_kerr_frame_device")


def kerr_frame(bh, dk, cfg, cam, width, height, flags=0, fields=KERR_FIELDS, diag=False):
    """bhrt_kerr_frame into host numpy arrays (with diag: h_residual and lz_drift as well)."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    extra, kd = _kerr_host_diag(width * height, diag)
    _check(load().bhrt_kerr_frame(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height, flags,
                                  C.byref(soa), _ptr(kd)), "bhrt_kerr_frame")
    arrays.update(extra)
    return arrays


def kerr_rays_device(rays_ptr, n, bh, dk, cfg, flags, soa, diag=None, stream=None):
    """bhrt_kerr_rays_device: n device rays (AoS) into device SoA buffers on a hipStream_t."""
    _check(load().bhrt_kerr_rays_device(C.c_void_p(rays_ptr), n, _ptr(bh), _ptr(dk), _ptr(cfg),
                                        flags, C.byref(soa), _ptr(diag),
                                        C.c_void_p(stream) if stream else None),
           "bhrt_kerr_rays_device")


def kerr_rays(rays, bh, dk, cfg, flags=0, fields=KERR_FIELDS, diag=False):
    """bhrt_kerr_rays: rays is a numpy array of abi.RAY_DTYPE; host numpy arrays back."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    arrays, soa = abi.alloc_soa(len(rays), fields)
    extra, kd = _kerr_host_diag(len(rays), diag)
    _check(load().bhrt_kerr_rays(rays.ctypes.data, len(rays), _ptr(bh), _ptr(dk), _ptr(cfg), flags,
                                 C.byref(soa), _ptr(kd)), "bhrt_kerr_rays")
    arrays.update(extra)
    return arrays


def _kerr_rk45_host_diag(n, diag):
    if not diag:
        return {}, None
    arrays = {"h_residual": np.zeros(n), "lz_drift": np.zeros(n),
              "rejected": np.zeros(n, dtype=np.int32)}
    return arrays, abi.KerrRk45Diag(*(arrays[f].ctypes.data
                                      for f in ("h_residual", "lz_drift", "rejected")))


def kerr_rk45_frame_device(bh, dk, cfg, cam, width, height, rows, flags, soa, diag=None,
                           stream=None):
    """bhrt_kerr_rk45_frame_device: kerr_frame_device with adaptive Dormand-Prince 5(4) steps
    under cfg.tolerance; diag an abi.KerrRk45Diag of device pointers or None."""
    _check(load().bhrt_kerr_rk45_frame_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                              height, _ptr(rows), flags, C.byref(soa), _ptr(diag),
                                              C.c_void_p(stream) if stream else None),
           "bhrt_kerr_rk45_frame_device")


def kerr_rk45_frame(bh, dk, cfg, cam, width, height, flags=0, fields=KERR_FIELDS, diag=False):
    """bhrt_kerr_rk45_frame into host numpy arrays (with diag: h_residual, lz_drift and rejected
    as well)."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    extra, kd = _kerr_rk45_host_diag(width * height, diag)
    _check(load().bhrt_kerr_rk45_frame(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height,
                                       flags, C.byref(soa), _ptr(kd)), "bhrt_kerr_rk45_frame")
    arrays.update(extra)
    return arrays


def kerr_rk45_rays_device(rays_ptr, n, bh, dk, cfg, flags, soa, diag=None, stream=None):
    """bhrt_kerr_rk45_rays_device: n device rays (AoS) into device SoA buffers on a hipStream_t."""
    _check(load().bhrt_kerr_rk45_rays_device(C.c_void_p(rays_ptr), n, _ptr(bh), _ptr(dk),
                                             _ptr(cfg), flags, C.byref(soa), _ptr(diag),
                                             C.c_void_p(stream) if stream else None),
           "bhrt_kerr_rk45_rays_device")


def kerr_rk45_rays(rays, bh, dk, cfg, flags=0, fields=KERR_FIELDS, diag=False):
    """bhrt_kerr_rk45_rays: rays is a numpy array of abi.RAY_DTYPE; host numpy arrays back."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    arrays, soa = abi.alloc_soa(len(rays), fields)
    extra, kd = _kerr_rk45_host_diag(len(rays), diag)
    _check(load().bhrt_kerr_rk45_rays(rays.ctypes.data, len(rays), _ptr(bh), _ptr(dk), _ptr(cfg),
                                      flags, C.byref(soa), _ptr(kd)), "bhrt_kerr_rk45_rays")
    arrays.update(extra)
    return arrays


def _kerr_emit_host(n, params, fill):
    """Host arrays of a bhrt_kerr_emit_out for n rays (radius, redshift [K, n] holding `fill`) and
    the struct pointing at them."""
    K = int(params.max_crossings) if params is not None else 1
    K = min(max(K, 1), abi.EMIT_MAX_CROSSINGS)     # (a refused K still gets arrays to point at)
    arrays = {"count": np.zeros(n, dtype=np.int32), "radius": np.full((K, n), fill, dtype=np.float64),
              "redshift": np.full((K, n), fill, dtype=np.float64), "intensity": np.zeros(n)}
    return arrays, abi.KerrEmitOut(*(arrays[f].ctypes.data for f in abi.EMIT_FIELDS))


def kerr_emit_frame_device(bh, dk, cfg, cam, width, height, rows, flags, soa, params, emit,
                           diag=None, stream=None):
    """bhrt_kerr_emit_frame_device: kerr_rk45_frame_device with up to params.max_crossings recorded
    disk crossings per ray; emit an abi.KerrEmitOut of device pointers (or None), diag an
    abi.KerrRk45Diag or None."""
    _check(load().bhrt_kerr_emit_frame_device(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width,
                                              height, _ptr(rows), flags, _ptr(soa), _ptr(diag),
                                              _ptr(params), _ptr(emit),
                                              C.c_void_p(stream) if stream else None),
           "bhrt_kerr_emit_frame_device")


def kerr_emit_frame(bh, dk, cfg, cam, width, height, params, flags=0, fields=KERR_FIELDS,
                    diag=False, fill=np.nan):
    """bhrt_kerr_emit_frame into host numpy arrays: the frame fields asked for, count, radius and
    redshift [K, n] (elements beyond a ray's count keep `fill`), intensity, and with diag
    h_residual, lz_drift and rejected."""
    arrays, soa = abi.alloc_soa(width * height, fields)
    extra, kd = _kerr_rk45_host_diag(width * height, diag)
    em, eo = _kerr_emit_host(width * height, params, fill)
    _check(load().bhrt_kerr_emit_frame(_ptr(bh), _ptr(dk), _ptr(cfg), _ptr(cam), width, height,
                                       flags, C.byref(soa), _ptr(kd), _ptr(params), C.byref(eo)),
           "bhrt_kerr_emit_frame")
    arrays.update(extra)
    arrays.update(em)
    return arrays


def kerr_emit_rays_device(rays_ptr, n, bh, dk, cfg, flags, soa, params, emit, diag=None,
                          stream=None):
    """bhrt_kerr_emit_rays_device: n device rays (AoS) into device buffers on a hipStream_t."""
    _check(load().bhrt_kerr_emit_rays_device(C.c_void_p(rays_ptr), n, _ptr(bh), _ptr(dk),
                                             _ptr(cfg), flags, _ptr(soa), _ptr(diag), _ptr(params),
                                             _ptr(emit), C.c_void_p(stream) if stream else None),
           "bhrt_kerr_emit_rays_device")


def kerr_emit_rays(rays, bh, dk, cfg, params, flags=0, fields=KERR_FIELDS, diag=False,
                   fill=np.nan):
    """bhrt_kerr_emit_rays: rays is a numpy array of abi.RAY_DTYPE; host numpy arrays back."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    arrays, soa = abi.alloc_soa(len(rays), fields)
    extra, kd = _kerr_rk45_host_diag(len(rays), diag)
    em, eo = _kerr_emit_host(len(rays), params, fill)
    _check(load().bhrt_kerr_emit_rays(rays.ctypes.data, len(rays), _ptr(bh), _ptr(dk), _ptr(cfg),
                                      flags, C.byref(soa), _ptr(kd), _ptr(params), C.byref(eo)),
           "bhrt_kerr_emit_rays")
    arrays.update(extra)
    arrays.update(em)
    return arrays


def kerr_disk_redshift(bh, radius, E, lz):
    """bhrt_kerr_disk_redshift: g = E_obs / E_emit of a disk crossing at Boyer-Lindquist `radius`
    for a photon with constants E and lz, on the host (0 where no circular orbit exists)."""
    g = C.c_double()
    _check(load().bhrt_kerr_disk_redshift(_ptr(bh), float(radius), float(E), float(lz),
                                          C.byref(g)), "bhrt_kerr_disk_redshift")
    return g.value


def kerr_paths_device(rays_ptr, n, bh, dk, cfg, max_positions, every, flags, paths, hits=None,
                      diag=None, stream=None):
    """bhrt_kerr_paths_device: the recorded Kerr geodesics of n device rays (AoS Ray[n] at
    rays_ptr) into the device arrays of `paths` (abi.Paths) and, if not None, the hit records of
    `hits` (abi.FrameSoA) and `diag` (abi.KerrDiag), asynchronous on a hipStream_t (int handle or
    None)."""
    _check(load().bhrt_kerr_paths_device(C.c_void_p(rays_ptr), int(n), _ptr(bh), _ptr(dk),
                                         _ptr(cfg), int(max_positions), int(every), int(flags),
                                         _ptr(paths), _ptr(hits), _ptr(diag),
                                         C.c_void_p(stream) if stream else None),
           "bhrt_kerr_paths_device")


def kerr_paths(rays, bh, dk, cfg, max_positions=abi.KERR_PATHS_DEFAULT_POSITIONS, every=1, flags=0,
               f32=False, fill=np.nan, fields=abi.KERR_PATH_HIT_FIELDS, diag=False):
    """bhrt_kerr_paths into host numpy arrays: rays is a numpy array of abi.RAY_DTYPE. Returns a
    dict with `xyz` [n, max_positions, 3] (float32 with f32, else float64; elements beyond a
    ray's count keep `fill`), `count` [n], the hit fields asked for (`fields`, any of
    KERR_FIELDS; empty: no hit records) and with diag h_residual and lz_drift."""
    rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE)
    n = len(rays)
    xyz = np.full((n, int(max_positions), 3), fill, dtype=np.float32 if f32 else np.float64)
    count = np.zeros(n, dtype=np.int32)
    paths = abi.Paths(xyz=None if f32 else xyz.ctypes.data, xyz32=xyz.ctypes.data if f32 else None,
                      count=count.ctypes.data)
    arrays, soa = abi.alloc_soa(n, fields) if fields else ({}, None)
    extra, kd = _kerr_host_diag(n, diag)
    _check(load().bhrt_kerr_paths(rays.ctypes.data, n, _ptr(bh), _ptr(dk), _ptr(cfg),
                                  int(max_positions), int(every), int(flags), C.byref(paths),
                                  _ptr(soa), _ptr(kd)), "bhrt_kerr_paths")
    arrays.update(extra)
    arrays["xyz"] = xyz
    arrays["count"] = count
    return arrays


def kerr_ray_init(bh, origin, direction):
    """bhrt_kerr_ray_init: (state [6] = (x, p), E) of one ray, on the host."""
    state = (C.c_double * 6)()
    E = C.c_double()
    o, d = abi.v3(*origin), abi.v3(*direction)
    _check(load().bhrt_kerr_ray_init(_ptr(bh), C.byref(o), C.byref(d), C.byref(state), C.byref(E)),
           "bhrt_kerr_ray_init")
    return np.array(state[:]), E.value


def particles_kerr_update_device(ps, bh, cfg, steps=1, params=None, diag=None, stream=None):
    """bhrt_particles_kerr_update_device: `steps` ticks of the resident array along timelike Kerr
    geodesics (abi.KerrParticlesParams; None: substeps 1), the diagnostics into the device arrays
    of `diag` (abi.KerrParticlesDiag or None), asynchronous on a hipStream_t (int handle or
    None)."""
    if params is None:
        params = abi.KerrParticlesParams()
    _check(load().bhrt_particles_kerr_update_device(ps, _ptr(bh), _ptr(cfg), int(steps),
                                                    _ptr(params), _ptr(diag),
                                                    C.c_void_p(stream) if stream else None),
           "bhrt_particles_kerr_update_device")


def kerr_particle_state(bh, position, velocity):
    """bhrt_kerr_particle_state: (state [6] = (x, p), E, u^t) of a unit-mass particle with
    coordinate velocity `velocity` at `position`, on the host; None where it is not timelike or
    lies inside the horizon."""
    state = (C.c_double * 6)()
    E, ut = C.c_double(), C.c_double()
    x, v = abi.v3(*position), abi.v3(*velocity)
    rc = load().bhrt_kerr_particle_state(_ptr(bh), C.byref(x), C.byref(v), C.byref(state),
                                         C.byref(E), C.byref(ut))
    if rc == 1:
        return None
    _check(rc, "bhrt_kerr_particle_state")
    return np.array(state[:]), E.value, ut.value


def kerr_orbit_velocity(bh, position, prograde=True):
    """bhrt_kerr_orbit_velocity: the coordinate velocity [3] of the circular equatorial geodesic
    through `position` (z == 0); None where no timelike circular orbit exists."""
    x, v = abi.v3(*position), abi.Vector3D()
    rc = load().bhrt_kerr_orbit_velocity(_ptr(bh), C.byref(x), 1 if prograde else 0, C.byref(v))
    if rc == 1:
        return None
    _check(rc, "bhrt_kerr_orbit_velocity")
    return np.array([v.x, v.y, v.z])


def set_claim_order(d_order_ptr, n):
    """bhrt_set_claim_order: the claim order (device int32 permutation of [0, n)) of this
    thread's next device camera frames of n rays; None / 0 = the default order. Raises if the
    array is not a permutation of [0, n)."""
    _check(load().bhrt_set_claim_order(d_order_ptr, int(n)), "bhrt_set_claim_order")


def check_guard_words(a_ptr, b_ptr, n, kind, out_ptr, stream):
    """bhrt_check_guard_words on device pointers: out[2i] = the high-word filter's answer,
    out[2i+1] = the exact test's (int32). Returns the call's status (0, or a hipError_t value)."""
    return load().bhrt_check_guard_words(a_ptr, b_ptr, int(n), int(kind), out_ptr, stream)


def shard_rows(height, rows):
    return load().bhrt_shard_rows(height, C.byref(rows))


def stats(reset=False):
    s = abi.Stats()
    _check(load().bhrt_get_stats(C.byref(s), 1 if reset else 0), "bhrt_get_stats")
    return {f: getattr(s, f) for f, _ in abi.Stats._fields_}


def stats_discard():
    """bhrt_get_stats(NULL, 1): wait for this thread's launches and drop their counters unread
    (no event timing: the cheap reset before a timed region)."""
    _check(load().bhrt_get_stats(None, 1), "bhrt_get_stats")


def halton(index, base):
    """halton_sequence (raytracer.c:852-863), libbhrt's host export."""
    L = load()
    L.halton_sequence.restype = C.c_double
    L.halton_sequence.argtypes = [C.c_int, C.c_int]
    return L.halton_sequence(index, base)
