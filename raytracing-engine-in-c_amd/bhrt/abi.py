"""ctypes mirror of include/bhrt_types.h and the bhrt_* extension structs of include/bhrt_api.h.

Pure data definitions: usable against libbhrt.so (the product), the oracle
(oracle/liboracle.so) and the compiled reference driver (oracle/_ref/libref.so), which all
share the reference's ABI (blackhole_types.h:15-115, raytracer.h:16-106).
"""
import ctypes as C

import numpy as np

RAY_HORIZON, RAY_DISK, RAY_BACKGROUND, RAY_MAX_DISTANCE, RAY_MAX_STEPS, RAY_ERROR = range(6)
INTEGRATOR_RK4, INTEGRATOR_RKF45, INTEGRATOR_LEAPFROG, INTEGRATOR_YOSHIDA = range(4)
JITTER_NONE, JITTER_REGULAR_GRID, JITTER_RANDOM, JITTER_HALTON, JITTER_BLUE_NOISE = range(5)
BHRT_FLAG_DOPPLER = 1
BHRT_FLAG_SKY = 2      # non-disk, non-horizon colours from the thread's bound sky map
BHRT_SKY_RGB32F = 0    # bhrt_sky_create formats: [H][W][3] float32
BHRT_SKY_RGBA8 = 1     # [H][W][4] uint8, alpha ignored


class Vector3D(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class Vector4D(C.Structure):
    _fields_ = [("t", C.c_double), ("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class Ray(C.Structure):
    _fields_ = [("origin", Vector3D), ("direction", Vector3D)]


class SchwarzschildMetric(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("g_tt", "g_rr", "g_thth", "g_phph")]


class BlackHoleParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "mass", "schwarzschild_radius", "spin", "charge", "r_plus", "r_minus",
        "isco_radius", "ergosphere_radius")]


class AccretionDiskParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "inner_radius", "outer_radius", "temperature_scale", "density_scale",
        "thickness_factor", "alpha_viscosity")]


class SimulationConfig(C.Structure):
    _fields_ = [("time_step", C.c_double), ("max_ray_distance", C.c_double),
                ("max_integration_steps", C.c_int), ("tolerance", C.c_double),
                ("use_adaptive_step", C.c_int), ("use_gpu_raytracing", C.c_int),
                ("doppler_factor", C.c_double), ("hawking_temp_factor", C.c_double),
                ("enable_doppler", C.c_int), ("enable_gravitational_redshift", C.c_int),
                ("show_accretion_disk", C.c_int)]


class SupersamplingParams(C.Structure):
    _fields_ = [("samples_per_pixel", C.c_int), ("jitter_method", C.c_int),
                ("jitter_strength", C.c_double)]


class AdaptiveSamplingParams(C.Structure):
    _fields_ = [("enable_adaptive", C.c_int), ("min_samples", C.c_int),
                ("max_samples", C.c_int), ("convergence_threshold", C.c_double),
                ("edge_threshold", C.c_double)]


class RayTraceHit(C.Structure):
    _fields_ = [("result", C.c_int), ("hit_position", Vector3D), ("hit_normal", Vector3D),
                ("distance", C.c_double), ("steps", C.c_int), ("time_dilation", C.c_double),
                ("sky_direction", Vector3D), ("doppler_factor", C.c_double),
                ("temperature", C.c_double), ("color", C.c_double * 3),
                ("redshift", C.c_double), ("optical_depth", C.c_double)]


class GPUShaderParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "mass", "spin", "schwarzschild_radius", "disk_inner_radius", "disk_outer_radius",
        "disk_temp_scale", "observer_distance", "fov")]


class Camera(C.Structure):
    _fields_ = [("position", Vector3D), ("direction", Vector3D), ("up", Vector3D),
                ("fov_deg", C.c_double), ("use_offset", C.c_int), ("offset_x", C.c_double),
                ("offset_y", C.c_double)]


class Rows(C.Structure):
    _fields_ = [("row_block", C.c_int), ("shard", C.c_int), ("num_shards", C.c_int)]


SOA_FIELDS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "time_dilation",
              "sky_x", "sky_y", "sky_z", "rgb_r", "rgb_g", "rgb_b")
SOA_DTYPES = {f: (np.int32 if f in ("result", "steps") else np.float64) for f in SOA_FIELDS}
# display path: 4 values per pixel (bhrt_frame_soa.rgba32f / rgba8)
DISPLAY_FIELDS = ("rgba32f", "rgba8")
SOA_DTYPES.update(rgba32f=np.float32, rgba8=np.uint8)


def rgba8_from_rgb(r, g, b):
    """The display conversion of bhrt_frame_soa.rgba8 in numpy (renderer.cpp:2090-2125):
    (unsigned char)(std::min(1.0f, (float)v) * 255.0f) per channel (NaN -> 255, truncation),
    alpha 255. Returns uint8 [n, 4]."""
    out = np.empty(np.shape(r) + (4,), dtype=np.uint8)
    for i, v in enumerate((r, g, b)):
        f = np.asarray(v).astype(np.float32)
        with np.errstate(invalid="ignore"):
            m = np.where(f < np.float32(1.0), f, np.float32(1.0))
        out[..., i] = (m * np.float32(255.0)).astype(np.uint8)
    out[..., 3] = 255
    return out


class FrameSoA(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in SOA_FIELDS + DISPLAY_FIELDS]


class Paths(C.Structure):
    """bhrt_paths: xyz [n][P] Vector3D, xyz32 [n][P][3] float, count [n] int32; 0 = not produced."""
    _fields_ = [("xyz", C.c_void_p), ("xyz32", C.c_void_p), ("count", C.c_void_p)]


PATHS_MAX_POSITIONS = 65536  # BHRT_PATHS_MAX_POSITIONS
# the hit fields a path launch produces (no colour or display field)
PATH_HIT_FIELDS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "time_dilation",
                   "sky_x", "sky_y", "sky_z")
# bhrt_kerr_paths: the hit fields the wrapper asks for by default (any field but time_dilation is
# allowed, the colours included), and its default max_positions
KERR_PATH_HIT_FIELDS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance")
KERR_PATHS_DEFAULT_POSITIONS = 1001


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("iterations", C.c_uint64), ("stages_full", C.c_uint64),
                ("stages_far", C.c_uint64), ("stages_kerr", C.c_uint64),
                ("launches", C.c_uint64), ("kernel_ms", C.c_double),
                ("rays_redone", C.c_uint64), ("span_ms", C.c_double),
                ("redo_launches", C.c_uint64), ("frame_ms", C.c_double),
                ("frame_ms_max", C.c_double), ("frames_timed", C.c_uint64),
                ("attempts_untested", C.c_uint64)]


class AdaptiveInfo(C.Structure):
    """bhrt_adaptive_info: what one adaptive frame did (include/bhrt_api.h)."""
    _fields_ = [("pixels", C.c_int64), ("edge_pixels", C.c_int64), ("sample_rays", C.c_int64),
                ("halo_pixels", C.c_int64)]


# temporal accumulation (include/bhrt_api.h)
BHRT_ACCUM_REFERENCE, BHRT_ACCUM_MEAN = 0, 1


class AccumParams(C.Structure):
    """bhrt_accum_params; AccumParams() holds the defaults of initTemporalBuffer."""
    _fields_ = [("schedule", C.c_int32), ("blend_factor", C.c_float), ("max_frames", C.c_int32),
                ("edge_threshold", C.c_float), ("edge_decay", C.c_float)]

    def __init__(self, schedule=BHRT_ACCUM_REFERENCE, blend_factor=0.1, max_frames=32,
                 edge_threshold=0.1, edge_decay=0.2):
        super().__init__(schedule, blend_factor, max_frames, edge_threshold, edge_decay)


class AccumState(C.Structure):
    """bhrt_accum_state: the host-side state of an accumulator."""
    _fields_ = [("frame_count", C.c_int32), ("jitter_index", C.c_int32),
                ("reset_pending", C.c_int32), ("cycle", C.c_int32), ("next_alpha", C.c_float),
                ("sharded", C.c_int32), ("next_offset_x", C.c_double),
                ("next_offset_y", C.c_double), ("frames_total", C.c_int64),
                ("pixels", C.c_int64)]


class AccumOut(C.Structure):
    """bhrt_accum_out: rgba8 [n][4] uint8, rgb [n][3] float32, edge_factor [n] float32."""
    _fields_ = [("rgba8", C.c_void_p), ("rgb", C.c_void_p), ("edge_factor", C.c_void_p)]


# numpy view of RayTraceHit (160 B, offsets pinned in include/bhrt_types.h)
HIT_DTYPE = np.dtype({
    "names": ["result", "hit_position", "hit_normal", "distance", "steps", "time_dilation",
              "sky_direction", "doppler_factor", "temperature", "color", "redshift",
              "optical_depth"],
    "formats": [np.int32, (np.float64, 3), (np.float64, 3), np.float64, np.int32, np.float64,
                (np.float64, 3), np.float64, np.float64, (np.float64, 3), np.float64, np.float64],
    "offsets": [0, 8, 32, 56, 64, 72, 80, 104, 112, 120, 144, 152],
    "itemsize": 160})
RAY_DTYPE = np.dtype([("origin", np.float64, 3), ("direction", np.float64, 3)])

# particle_sim.h:15-75 (Particle 152 B, ParticleSystem 32 B; pinned in bhrt_types.h)
PARTICLE_TEST, PARTICLE_DISK, PARTICLE_HAWKING, PARTICLE_JET = 0, 1, 2, 3


class Particle(C.Structure):
    _fields_ = [("position", Vector3D), ("velocity", Vector3D), ("acceleration", Vector3D),
                ("mass", C.c_double), ("energy", C.c_double), ("angular_momentum", C.c_double),
                ("proper_time", C.c_double), ("coordinate_time", C.c_double),
                ("type", C.c_int), ("active", C.c_int), ("id", C.c_int), ("age", C.c_double),
                ("temperature", C.c_double), ("time_dilation", C.c_double)]


class ParticleSystem(C.Structure):
    _fields_ = [("particles", C.POINTER(Particle)), ("capacity", C.c_int), ("count", C.c_int),
                ("next_id", C.c_int), ("blackhole", C.c_void_p)]


PARTICLE_DTYPE = np.dtype({
    "names": ["position", "velocity", "acceleration", "mass", "energy", "angular_momentum",
              "proper_time", "coordinate_time", "type", "active", "id", "age", "temperature",
              "time_dilation"],
    "formats": [(np.float64, 3), (np.float64, 3), (np.float64, 3)] + [np.float64] * 5 +
               [np.int32] * 3 + [np.float64] * 3,
    "offsets": [0, 24, 48, 72, 80, 88, 96, 104, 112, 116, 120, 128, 136, 144],
    "itemsize": 152})


def particles_view(ps):
    """numpy view (no copy) of ps.particles[0:count]."""
    if ps.count <= 0:
        return np.zeros(0, dtype=PARTICLE_DTYPE)
    buf = (C.c_char * (ps.count * 152)).from_address(C.addressof(ps.particles.contents))
    return np.frombuffer(buf, dtype=PARTICLE_DTYPE)


PARTICLE_DATA_FIELDS = ("positions", "velocities", "types", "ids", "xyz32", "vel32", "count")
# per element of bhrt_particle_data: (trailing shape, dtype)
PARTICLE_DATA_SHAPES = {"positions": ((3,), np.float64), "velocities": ((3,), np.float64),
                        "types": ((), np.int32), "ids": ((), np.int32),
                        "xyz32": ((3,), np.float32), "vel32": ((3,), np.float32)}


class ParticleData(C.Structure):
    """bhrt_particle_data: device (or host) arrays of max_count elements, count [1]; any None."""
    _fields_ = [(f, C.c_void_p) for f in PARTICLE_DATA_FIELDS]


class SkyState(C.Structure):
    """bhrt_sky_state: a sky map's size, input format and device."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32),
                ("device", C.c_int32)]


class KerrDiag(C.Structure):
    """bhrt_kerr_diag: optional per-ray arrays (device or host, as the call's outputs); 0 = not
    produced."""
    _fields_ = [("h_residual", C.c_void_p), ("lz_drift", C.c_void_p)]


class KerrRk45Diag(C.Structure):
    """bhrt_kerr_rk45_diag: KerrDiag's arrays and rejected (int32 per ray); 0 = not produced."""
    _fields_ = [("h_residual", C.c_void_p), ("lz_drift", C.c_void_p), ("rejected", C.c_void_p)]


EMIT_MAX_CROSSINGS = 4  # BHRT_EMIT_MAX_CROSSINGS


class KerrEmitParams(C.Structure):
    """bhrt_kerr_emit_params: K = max_crossings (1..EMIT_MAX_CROSSINGS), the emissivity's index q
    of eps(r) = (inner_radius / r)^q, and the colour's gain."""
    _fields_ = [("max_crossings", C.c_int), ("emissivity_index", C.c_double), ("gain", C.c_double)]

    def __init__(self, max_crossings=1, emissivity_index=3.0, gain=1.0):
        super().__init__(max_crossings, emissivity_index, gain)


EMIT_FIELDS = ("count", "radius", "redshift", "intensity")


class KerrEmitOut(C.Structure):
    """bhrt_kerr_emit_out: count [n] int32, radius and redshift [K][n], intensity [n] (device or
    host, as the call's outputs); 0 = not produced."""
    _fields_ = [(f, C.c_void_p) for f in EMIT_FIELDS]


# BHRT_PSTAT_*: what bhrt_particles_kerr_update_device did with a particle
PSTAT_MOVED, PSTAT_CAPTURED, PSTAT_NOT_TIMELIKE, PSTAT_ERROR, PSTAT_INACTIVE = 0, 1, 2, 3, 4
KERR_PARTICLES_MAX_SUBSTEPS = 64


class KerrParticlesParams(C.Structure):
    """bhrt_kerr_particles_params: substeps (1..64), the RK4 substeps of a tick far from the hole."""
    _fields_ = [("substeps", C.c_int)]

    def __init__(self, substeps=1):
        super().__init__(substeps)


KERR_PARTICLES_DIAG_FIELDS = ("h_residual", "lz_drift", "status", "substeps")
KERR_PARTICLES_DIAG_DTYPES = {"h_residual": np.float64, "lz_drift": np.float64,
                              "status": np.int32, "substeps": np.int32}


class KerrParticlesDiag(C.Structure):
    """bhrt_kerr_particles_diag: optional DEVICE arrays [count] by array index; 0 = not produced."""
    _fields_ = [(f, C.c_void_p) for f in KERR_PARTICLES_DIAG_FIELDS]


class ParticlesState(C.Structure):
    """bhrt_particles_state: the host-side state of a device-resident particle system."""
    _fields_ = [("count", C.c_int32), ("device", C.c_int32), ("updates", C.c_int64)]


assert C.sizeof(Particle) == 152 and C.sizeof(ParticleSystem) == 32
assert C.sizeof(RayTraceHit) == 160 and C.sizeof(SimulationConfig) == 72
assert C.sizeof(BlackHoleParams) == 64 and C.sizeof(AccretionDiskParams) == 48


def v3(x, y, z):
    return Vector3D(float(x), float(y), float(z))


def alloc_soa(n, fields=SOA_FIELDS):
    """Host SoA arrays (numpy) + the FrameSoA struct pointing at them."""
    arrays = {f: np.zeros((n, 4) if f in DISPLAY_FIELDS else n, dtype=SOA_DTYPES[f])
              for f in fields}
    soa = FrameSoA(**{f: a.ctypes.data for f, a in arrays.items()})
    return arrays, soa


def _isco(mass, spin):
    """get_isco_radius (spacetime.c:285-308), used only to build configs."""
    import math
    M, a = mass, spin * mass
    if spin == 0.0:
        return 6.0 * M
    z1 = 1.0 + pow(1.0 - a * a / (M * M), 1.0 / 3.0) * (
        pow(1.0 + a / M, 1.0 / 3.0) + pow(1.0 - a / M, 1.0 / 3.0))
    z2 = math.sqrt(3.0 * a * a / (M * M) + z1 * z1)
    return M * (3.0 + z2 - math.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)))


def black_hole(mass=1.0, spin=0.0, charge=0.0):
    """initialize_black_hole_params (spacetime.c:331-366), for spin >= 0, charge == 0."""
    import math
    bh = BlackHoleParams()
    bh.mass, bh.spin, bh.charge = mass, spin, charge
    bh.schwarzschild_radius = 2.0 * mass
    if spin == 0.0 and charge == 0.0:
        bh.r_plus, bh.r_minus, bh.ergosphere_radius = 2.0 * mass, 0.0, 2.0 * mass
    else:
        a = spin * mass
        s = math.sqrt(mass * mass - a * a - charge * charge)
        bh.r_plus, bh.r_minus, bh.ergosphere_radius = mass + s, mass - s, 2.0 * mass
    bh.isco_radius = _isco(mass, spin)
    return bh


def disk(inner, outer=20.0, tscale=1.0, density=1.0):
    d = AccretionDiskParams()
    d.inner_radius, d.outer_radius, d.temperature_scale, d.density_scale = inner, outer, tscale, density
    return d


def sim_config(time_step=0.1, max_dist=100.0, max_steps=1000, tol=1e-6):
    c = SimulationConfig()
    c.time_step, c.max_ray_distance, c.max_integration_steps, c.tolerance = (
        time_step, max_dist, max_steps, tol)
    return c
