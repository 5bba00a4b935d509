/*
 * bhrt_api.h -- C ABI of libbhrt.so, the MI355X geodesic ray tracer.
 *
 * Two groups of entry points:
 *
 *  1. Drop-in: the reference engine's own symbols, same names, arguments, return codes and
 *     struct layouts (bhrt_types.h). Each declaration names the reference interface it
 *     replaces. The ray-tracing ones (trace_ray, trace_rays_batch, integrate_photon_path,
 *     trace_pixel, bh_trace_ray, bh_trace_rays_batch) run on the GPU; there is no CPU
 *     fallback: if HIP is unavailable they return the reference's error value and
 *     bhrt_last_error() says why.
 *
 *  2. Extension (bhrt_*): whole-frame rendering with device-resident SoA outputs, row
 *     sharding for multi-GPU, and launch statistics. This is what bench.py drives.
 *
 * Host buffers are always caller-owned; nothing is retained across calls.
 */
#ifndef BHRT_API_H
#define BHRT_API_H

#include "bhrt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BLACKHOLE_API_VERSION_MAJOR 0
#define BLACKHOLE_API_VERSION_MINOR 1
#define BLACKHOLE_API_VERSION_PATCH 0

#define BH_PI 3.14159265358979323846
#define BH_EPSILON 1.0e-10
#define BH_TWO_PI 6.28318530717958647692

typedef enum {
    BH_SUCCESS = 0,
    BH_ERROR_INVALID_PARAMETER = -1,
    BH_ERROR_MEMORY_ALLOCATION = -2,
    BH_ERROR_INITIALIZATION = -3,
    BH_ERROR_SIMULATION = -4
} BHErrorCode; /* include/blackhole_api.h:30-36 */

typedef struct BHContext_t* BHContextHandle; /* include/blackhole_api.h:40 */

/* ================================ 1. drop-in symbols ==================================== */

/* --- ray tracing (GPU) --- */

/* replaces raytracer.h:129-133 / src/raytracer.c:684-767 */
RayTraceResult trace_ray(const Ray* ray, const BlackHoleParams* blackhole,
                         const AccretionDiskParams* disk, const SimulationConfig* config,
                         RayTraceHit* hit);

/* replaces raytracer.h:205-212 / src/raytracer.c:782-807. Returns -1 if rays, blackhole or
 * hits is NULL or num_rays <= 0, else 0. num_threads is ignored (the GPU decides). */
int trace_rays_batch(const Ray* rays, int num_rays, const BlackHoleParams* blackhole,
                     const AccretionDiskParams* disk, const SimulationConfig* config,
                     RayTraceHit* hits, int num_threads);

/* replaces raytracer.h:181-190 / src/raytracer.c:338-679 */
RayTraceResult integrate_photon_path(const Vector4D* position, const Vector3D* direction,
                                     const BlackHoleParams* blackhole,
                                     const SimulationConfig* config, IntegrationMethod method,
                                     Vector3D* path_positions, int max_positions,
                                     int* num_positions, RayTraceHit* hit);

/* replaces raytracer.h:151-165 / src/raytracer.c:1044-1167 (see DESIGN.md for the colour
 * of disk samples, which the reference reads from an uninitialised field) */
RayTraceResult trace_pixel(int pixel_x, int pixel_y, int width, int height,
                           const Vector3D* camera_position, const Vector3D* camera_direction,
                           const Vector3D* camera_up, double fov,
                           const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                           const SimulationConfig* config, const SupersamplingParams* ss_params,
                           const AdaptiveSamplingParams* as_params, double color_out[3]);

/* --- ray-path helpers (host scalar code, same arithmetic as the device) --- */
int check_disk_intersection(const Vector3D* position, const Vector3D* velocity,
                            const Vector3D* prev_position, const AccretionDiskParams* disk,
                            Vector3D* hit_position);                     /* raytracer.c:159 */
void calculate_disk_temperature(const Vector3D* position, const BlackHoleParams* blackhole,
                                const AccretionDiskParams* disk, double* temperature,
                                double color[3]);                        /* raytracer.c:201 */
void apply_relativistic_effects(const Vector3D* position, const Vector3D* velocity,
                                const BlackHoleParams* blackhole, double color[3],
                                double* doppler_factor);                 /* raytracer.c:233 */
void generate_gpu_shader_params(const BlackHoleParams* blackhole,
                                const AccretionDiskParams* disk, double observer_distance,
                                double fov, GPUShaderParams* params);     /* raytracer.c:818 */
double halton_sequence(int index, int base);                             /* raytracer.c:852 */

/* spacetime.h */
void initialize_black_hole_params(BlackHoleParams* blackhole, double mass, double spin,
                                  double charge);                        /* spacetime.c:331 */
double get_isco_radius(const BlackHoleParams* blackhole);                /* spacetime.c:285 */
SchwarzschildMetric calculate_schwarzschild_metric(double r, const BlackHoleParams* bh);
                                                                         /* spacetime.c:15 */
double calculate_time_dilation(double r, const BlackHoleParams* blackhole);/* spacetime.c:192 */
void cartesian_to_spherical(const Vector3D* cartesian, Vector3D* spherical);/* spacetime.c:201 */
void spherical_to_cartesian(const Vector3D* spherical, Vector3D* cartesian);/* spacetime.c:229 */
KerrMetric calculate_kerr_metric(double r, double theta, const BlackHoleParams* blackhole);
                                                                         /* spacetime.c:38 */
BlackHoleMetric calculate_metric(double r, double theta, const BlackHoleParams* blackhole);
                                                                         /* spacetime.c:74 */
double calculate_effective_potential(double r, double l, const BlackHoleParams* blackhole);
                                                                         /* spacetime.c:242 */
double calculate_ergosphere_radius(double theta, const BlackHoleParams* blackhole);
                                                                         /* spacetime.c:314 */
int calculate_kerr_metric_bl(const double position[4], double a, double M, KerrMetric* metric);
                                                                         /* spacetime.c:377 */
int calculate_inverse_kerr_metric(const double position[4], double a, double M,
                                  KerrMetric* inv_metric);               /* spacetime.c:429 */
int calculate_kerr_christoffel(const double position[4], double a, double M,
                               double christoffel[4][4][4]);             /* spacetime.c:483 */
double calculate_kerr_isco(double a, double M, bool prograde);           /* spacetime.c:548 */
double calculate_kerr_event_horizon(double a, double M);                 /* spacetime.c:565 */
double calculate_kerr_ergosphere(double a, double M, double theta);      /* spacetime.c:577 */
int calculate_frame_dragging(const double position[4], double a, double M, double velocity[3]);
                                                                         /* spacetime.c:590 */
int calculate_kerr_geodesic(const double position[4], const double velocity[4], double a,
                            double M, double acceleration[4]);           /* spacetime.c:624 */
void calculate_christoffel_symbols(double r, double theta, const BlackHoleParams* blackhole,
                                   double christoffel[4][4][4]);         /* spacetime.c:93 */
void geodesic_equation(const double position[4], const double velocity[4],
                       const BlackHoleParams* blackhole, double acceleration[4]);
                                                                         /* spacetime.c:166 */

/* math_util.h */
Vector3D vector3D_add(const Vector3D a, const Vector3D b);               /* math_util.c:31 */
Vector3D vector3D_sub(const Vector3D a, const Vector3D b);               /* math_util.c:49 */
Vector3D vector3D_scale(const Vector3D v, double scale);                 /* math_util.c:67 */
double   vector3D_dot(const Vector3D a, const Vector3D b);               /* math_util.c:85 */
Vector3D vector3D_cross(const Vector3D a, const Vector3D b);             /* math_util.c:100 */
double   vector3D_length(const Vector3D v);                              /* math_util.c:111 */
Vector3D vector3D_normalize(const Vector3D v);                           /* math_util.c:115 */
void rk4_integrate(ODEFunction f, double* y, int n, double t, double h, void* params);
                                                                         /* math_util.c:162 */
int rkf45_integrate(ODEFunction f, double y[], int n, double* t, double h_try, double* h_next,
                    double eps_rel, void* params);                       /* math_util.c:212 */
void temperature_to_rgb(double temperature, double rgb[3]);              /* math_util.c:463 */
double clamp(double value, double min, double max);                      /* math_util.c:505 */
void leapfrog_integrate(ODEFunctionSecondOrder f, double* x, double* v, int n, double t,
                        double dt, void* params);                        /* math_util.c:125 */

/* particle_sim.h -- host bookkeeping; update_particles runs on the GPU (one lane per
 * particle). */
int particle_system_init(ParticleSystem* system, int initial_capacity);   /* particle_sim.c:73 */
void particle_system_cleanup(ParticleSystem* system);                    /* particle_sim.c:96 */
int add_particle(ParticleSystem* system, const Vector3D* position, const Vector3D* velocity,
                 double mass, ParticleType type);                        /* particle_sim.c:108 */
int update_particles(ParticleSystem* system, const BlackHoleParams* blackhole,
                     const SimulationConfig* config);                    /* particle_sim.c:505 */
/* defined (non-static) by the reference but not declared in its headers */
Particle* find_particle(ParticleSystem* system, int particle_id);        /* particle_sim.c:138 */
int remove_particle(ParticleSystem* system, int particle_id);            /* particle_sim.c:155 */
int calculate_particle_orbit(const ParticleSystem* system, int particle_id,
                             const BlackHoleParams* blackhole, OrbitalParams* params);
                                                                         /* particle_sim.c:571 */
int calculate_circular_orbit(double r, const BlackHoleParams* blackhole, Vector3D* velocity);
                                                                         /* particle_sim.c:604 */
int create_accretion_disk(ParticleSystem* system, const BlackHoleParams* blackhole,
                          const AccretionDiskParams* disk, int num_particles);
                                                                         /* particle_sim.c:339 */
int generate_hawking_radiation(ParticleSystem* system, const BlackHoleParams* blackhole,
                               int num_particles, const SimulationConfig* config);
                                                                         /* particle_sim.c:427 */

/* --- context API (include/blackhole_api.h:47-255, src/blackhole_api.c) --- */
BHContextHandle bh_initialize(void);                                     /* blackhole_api.c:52 */
void bh_shutdown(BHContextHandle context);                               /* blackhole_api.c:85 */
double blackhole_get_mass(BHContextHandle context);                      /* blackhole_api.c:33 */
void bh_calculate_orbital_velocity(BHContextHandle context, double r, double* v_phi);
                                                                         /* blackhole_api.c:42 */
BHErrorCode bh_configure_black_hole(BHContextHandle context, double mass, double spin,
                                    double charge);                      /* blackhole_api.c:94 */
BHErrorCode bh_configure_accretion_disk(BHContextHandle context, double inner_radius,
                                        double outer_radius, double temperature_scale,
                                        double density_scale);           /* blackhole_api.c:123 */
BHErrorCode bh_configure_simulation(BHContextHandle context, double time_step,
                                    double max_ray_distance, int max_integration_steps,
                                    double tolerance);                   /* blackhole_api.c:153 */
BHErrorCode bh_trace_ray(BHContextHandle context, const double origin[3],
                         const double direction[3], RayTraceHit* hit);   /* blackhole_api.c:182 */
BHErrorCode bh_trace_rays_batch(BHContextHandle context, const Ray* rays, RayTraceHit* hits,
                                int count);                              /* blackhole_api.c:225 */
void* bh_create_particle_system(BHContextHandle context, int capacity); /* blackhole_api.c:256 */
void bh_destroy_particle_system(BHContextHandle context, void* system);  /* blackhole_api.c:280 */
int bh_add_test_particle(BHContextHandle context, void* system, const double position[3],
                         const double velocity[3], double mass);         /* blackhole_api.c:296 */
int bh_create_accretion_disk_particles(BHContextHandle context, void* system,
                                       int num_particles);               /* blackhole_api.c:318 */
int bh_generate_hawking_radiation(BHContextHandle context, void* system, int num_particles);
                                                                         /* blackhole_api.c:343 */
BHErrorCode bh_update_particles(BHContextHandle context, void* system);  /* blackhole_api.c:364 */
BHErrorCode bh_get_particle_data(BHContextHandle context, void* system, double* positions,
                                 double* velocities, int* types, int* count);
                                                                         /* blackhole_api.c:384 */
BHErrorCode bh_calculate_time_dilation(BHContextHandle context, const double position1[3],
                                       const double position2[3], double* time_ratio);
                                                                         /* blackhole_api.c:432 */
void bh_get_version(int* major, int* minor, int* patch);                 /* blackhole_api.c:464 */
BHErrorCode bh_generate_shader_data(void* context, const float observer_pos[3],
                                    const float observer_dir[3], const float up_vector[3],
                                    int width, int height, float fov, int enable_doppler,
                                    int enable_redshift, int show_disk, float* output_buffer);
                                                                         /* blackhole_api.c:495 */

/* ================================ 2. bhrt extension ===================================== */

/* Pinhole camera of trace_pixel/calculate_ray_direction (raytracer.c:999-1039); fov in
 * degrees. Rays go through the pixel centres (offset 0.5, 0.5) unless use_offset is set:
 * then every pixel uses (offset_x, offset_y), e.g. one sample of trace_pixel's jitter
 * (generate_jittered_position, raytracer.c:868-932). A zero-initialised tail means centres. */
typedef struct {
    Vector3D position;
    Vector3D direction;
    Vector3D up;
    double   fov_deg;
    int      use_offset;
    double   offset_x, offset_y;
} bhrt_camera;

/* Frame flags */
#define BHRT_FLAG_DOPPLER 1 /* disk colour through apply_relativistic_effects (config C4) */
#define BHRT_FLAG_SKY 2     /* non-disk, non-horizon rays take their colour from the calling
                               thread's bound sky map ("Sky maps" below) instead of the gradient */

/* Structure-of-arrays frame. Element i is the i-th ray of the launch (for a camera frame:
 * the i-th pixel of the shard, row-major over the shard's rows). Any pointer may be NULL,
 * in which case that field is not produced. Pointers are device pointers for the *_device
 * calls and host pointers otherwise. */
typedef struct {
    int32_t* result;        /* RayTraceResult                                            */
    int32_t* steps;         /* RayTraceHit.steps                                         */
    double*  hit_x;         /* RayTraceHit.hit_position                                  */
    double*  hit_y;
    double*  hit_z;
    double*  distance;
    double*  time_dilation;
    double*  sky_x;         /* RayTraceHit.sky_direction, written for MAX_DISTANCE only  */
    double*  sky_y;
    double*  sky_z;
    double*  rgb_r;         /* frame colour contract, DESIGN.md section 3                */
    double*  rgb_g;
    double*  rgb_b;
    /* display path (renderer.cpp:2090-2125, the visualizer's texture buffer): 4 values per
     * pixel, row 0 = top image row */
    float*   rgba32f;       /* (float)rgb and alpha 1.0f: the compute shader's RayOutput   */
    uint8_t* rgba8;         /* (unsigned char)(std::min(1.0f, v) * 255.0f) of rgba32f      */
} bhrt_frame_soa;

/* Cyclic row-block sharding of an image across num_shards GPUs: block b (rows
 * [b*row_block, (b+1)*row_block)) belongs to shard b % num_shards. {0,0,1} = whole image. */
typedef struct {
    int row_block;
    int shard;
    int num_shards;
} bhrt_rows;

/* Launch statistics accumulated on the calling thread since the last reset. */
typedef struct {
    uint64_t rays;          /* rays traced                                               */
    uint64_t iterations;    /* executed RK4 iterations / RKF45 attempts                  */
    uint64_t stages_full;   /* ray_derivatives evaluations, a=0 strong-field branch      */
    uint64_t stages_far;    /* ... far-field branch                                      */
    uint64_t stages_kerr;   /* ... spin != 0 branch                                      */
    uint64_t launches;      /* trace-kernel launches timed                               */
    double   kernel_ms;     /* sum of HIP-event durations of those launches              */
    uint64_t rays_redone;   /* rays re-traced on the large-argument sincos path          */
    double   span_ms;       /* per GPU: first trace-kernel start to last trace-kernel end
                               since the reset (summed over GPUs); launches overlapping on
                               several streams make this, not kernel_ms, the GPU time     */
    uint64_t redo_launches; /* of those launches, how many were followed by the redo pass
                               (left out where no ray can need it)   */
    /* per launch, the frame's execution window on the GPU's constant-rate wall clock: its
     * first trace wave's start to its last store (the trace kernel's last wave, or the separate
     * colour pass's last workgroup) -- the frame's completion latency once it runs */
    double   frame_ms;      /* sum over the timed launches                               */
    double   frame_ms_max;  /* the longest                                               */
    uint64_t frames_timed;  /* launches with a window (0 where the clock rate is unknown) */
    uint64_t attempts_untested; /* of `iterations`, the RKF45 attempts run without the error
                               estimate and accept test: launches where the host proved every
                               attempt passes (zero-acceleration paths)     */
} bhrt_stats;

/* Number of rows of an image of `height` rows owned by shard rows->shard. */
int bhrt_shard_rows(int height, const bhrt_rows* rows);

/* Render (a shard of) a camera frame into DEVICE SoA buffers on `hip_stream` (a
 * hipStream_t). Asynchronous: returns after the launch. hip_stream NULL behaves like a launch
 * on the legacy default stream: the frame is ordered after all work the caller queued there
 * (e.g. a hipMemset or a torch fill of the output arrays) and before all work queued there
 * afterwards (e.g. a hipMemcpy of the results); the kernels run on the library's per-thread
 * stream, linked to the default stream by two event waits. BHRT_NULL_STREAM=unordered drops
 * that ordering (the library's stream alone). Returns 0, or -1 on invalid arguments / HIP
 * failure (see bhrt_last_error). */
int bhrt_render_frame_device(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                             const SimulationConfig* config, const bhrt_camera* camera,
                             int width, int height, const bhrt_rows* rows,
                             IntegrationMethod method, int flags,
                             const bhrt_frame_soa* device_out, void* hip_stream);

/* One camera frame rendered by several GPUs and gathered on the calling thread's CURRENT device
 * (the root) -- the north star's "image tiled across the GPUs, one gather at frame end", from C:
 * the image is split into `shards` cyclic row-block shards of 8 rows (<= 0: one per device),
 * shard s rendered by device (root + s) mod ndev into that device's own buffers (ndev <= 0:
 * every visible device), and the root copies every shard straight into its image rows of
 * device_out -- device-to-device over xGMI for the peers (peer access enabled on first use),
 * one strided 2-D copy per field and shard. device_out: root-device buffers of width * height
 * elements per field (NULL fields are not produced). Asynchronous on hip_stream (a root-device
 * hipStream_t): the frame is complete when that stream's work is; NULL = ordered like the
 * root's legacy default stream, as for bhrt_render_frame_device. A
 * one-shard frame is bhrt_render_frame_device on the root. Replaces the reference's serial
 * per-pixel loop (raytracer.c:795-804 / blackhole_api.c:225-250) on a multi-GPU node. */
int bhrt_render_frame_gather(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                             const SimulationConfig* config, const bhrt_camera* camera,
                             int width, int height, IntegrationMethod method, int flags,
                             const bhrt_frame_soa* device_out, int ndev, int shards,
                             void* hip_stream);

/* Same, into HOST buffers; splits the image over every visible GPU (cyclic row blocks)
 * and returns when the frame is complete. */
int bhrt_render_frame(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                      const SimulationConfig* config, const bhrt_camera* camera, int width,
                      int height, IntegrationMethod method, int flags,
                      const bhrt_frame_soa* host_out);

/* ---- supersampled frames: every pixel is trace_pixel's sample average ---- */
#define BHRT_SS_MAX_SAMPLES 64

/* trace_pixel's sample count and sub-pixel offsets (raytracer.c:1066-1108, 868-932) for
 * these parameters: writes offset_x/y[0..count) and returns count (>= 1), or -1.
 * count = ss ? ss->samples_per_pixel : 1, or with as->enable_adaptive min_samples +
 * (int)((max_samples - min_samples) * 1.0) capped at max_samples (the reference's edge factor is
 * fixed at 1). Sample s lies at generate_jittered_position(s, ss->samples_per_pixel, ...) where
 * ss->samples_per_pixel > 1, else at the centre (0.5, 0.5) -- with the reference's quirks: the
 * grid is (int)sqrt(spp) wide (the fifth sample of a "2x2" grid lies at (0.25, 1.25), outside
 * the pixel), Halton sample 0 is (0, 0), JITTER_BLUE_NOISE is Halton, jitter_strength != 1
 * scales about the centre. -1 for JITTER_RANDOM with more than one sample per pixel (rand() per
 * pixel: not reproducible), a count below 1 or above BHRT_SS_MAX_SAMPLES, or above capacity. */
int bhrt_sample_offsets(const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                        double* offset_x, double* offset_y, int capacity);

/* (A shard of) a camera frame in which every pixel is trace_pixel(px, py, ..., ss, as), for any
 * method and flags: DEVICE buffers, asynchronous on hip_stream (NULL: ordered like the legacy
 * default stream, exactly as bhrt_render_frame_device). Of device_out only result (the class of
 * sample 0, trace_pixel's return value), rgb_r/g/b (all three), rgba32f and rgba8 may be
 * non-NULL. The pixel colour is ((...((0.0 + c_0) + c_1) + ...) + c_{S-1}) / S per channel in
 * IEEE double, trace_pixel's accumulation order, with no contraction and no atomics: a pure
 * function of the pixel's samples, the same bits run to run, on any stream and in any shard
 * split; one NaN sample makes the pixel NaN (rgba8 255). The S samples of all pixels are traced
 * by one launch of rays * S rays (bhrt_stats.rays counts them; bhrt_set_claim_order does not
 * apply) into per-stream scratch of about 228 B per sample ray -- 52 B of directions, colour
 * and class on top of the 176 B of launch scratch every ray has -- i.e. 1.9 GB for a 1920x1080
 * frame of 4 samples. Returns 0, or -1 (nothing written) for a bad bhrt_sample_offsets case,
 * camera->use_offset != 0, any other non-NULL field, rays * S > INT_MAX, or an allocation or
 * HIP failure (bhrt_last_error). */
int bhrt_render_frame_ss_device(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                                const SimulationConfig* config, const bhrt_camera* camera,
                                int width, int height, const bhrt_rows* rows,
                                IntegrationMethod method, int flags,
                                const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                                const bhrt_frame_soa* device_out, void* hip_stream);

/* The same whole frame into HOST arrays, on the current device; returns when it is complete. */
int bhrt_render_frame_ss(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                         const SimulationConfig* config, const bhrt_camera* camera, int width,
                         int height, IntegrationMethod method, int flags,
                         const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                         const bhrt_frame_soa* host_out);

/* ---- adaptive supersampled frames: max_samples only at edge pixels ---- */

/* What one adaptive frame did: the shard's pixels, how many of them are edge pixels, the rays
 * both passes traced (= what bhrt_stats.rays gains), and the pixels of other shards' rows that
 * were traced for the edge rule alone (0 for a whole image). */
typedef struct {
    int64_t pixels, edge_pixels, sample_rays, halo_pixels;
} bhrt_adaptive_info;

/* (A shard of) a camera frame that gives every pixel as->min_samples samples and only the edge
 * pixels as->max_samples. THE RULE, with B = as->min_samples, M = as->max_samples, o_s the first M
 * offsets of bhrt_sample_offsets(ss, as) and c_s(p) the colour of pixel p's sample s under the
 * frame colour contract:
 *  1. base(p) = ((...((0.0 + c_0) + c_1) + ...) + c_{B-1}) / B per channel, in IEEE double with
 *     no contraction;
 *  2. g(p) starts at 0.0; for each of the 4 neighbours q of p inside the IMAGE (not the shard)
 *     d = (|base_r(p) - base_r(q)| + |base_g(p) - base_g(q)| + |base_b(p) - base_b(q)|) / 3.0
 *     with no contraction, and if (d > g) g = d -- a NaN d never raises g, and image-border
 *     pixels use the neighbours they have;
 *  3. edge_factor(p) = g(p) > as->edge_threshold ? 1.0 : 0.0 (a NaN threshold: no edges; a
 *     negative threshold: every pixel an edge);
 *  4. S(p) is trace_pixel's count with that factor (raytracer.c:1074-1093): B, and where the
 *     factor exceeds 0.5 min(B + (int)((M - B) * factor), M) = M;
 *  5. the pixel is ((...((0.0 + c_0) + ...) + c_{S(p)-1}) / S(p): the running SUM continued, not
 *     the base mean re-weighted; its class is sample 0's, its display fields are the frame's
 *     conversions of it.
 * A pixel is a pure function of the image: the same bits run to run, on any stream and in any
 * row-shard split (a shard traces the base samples of the image rows next to its own, its halo,
 * for step 2; they are never output). With a negative threshold the frame is
 * bhrt_render_frame_ss_device's of M samples bit for bit, with +inf or NaN its frame of B.
 * DEVICE buffers: device_out as for bhrt_render_frame_ss_device (result, all three of
 * rgb_r/g/b, rgba32f, rgba8), device_samples (may be NULL) S(p) per shard pixel; info (HOST, may
 * be NULL) is filled before the call returns.
 * Two trace launches on hip_stream (NULL: ordered like the legacy default stream): the base
 * samples, then the edge pixels' extra samples (none where there is no edge pixel or M == B).
 * The size of the second is known only on the device, so the call reads the edge count with one
 * 8-byte copy and WAITS on the host for the base pass: it is asynchronous only from the second
 * pass on, and two frames in flight need two host threads or the caller's own interleaving.
 * bhrt_stats.rays gains info->sample_rays; bhrt_set_claim_order does not apply. Scratch: about
 * 228 B per base ray (halo included) plus as much per extra ray, in two per-stream blocks.
 * Returns 0, or -1 with nothing written (bhrt_last_error) for everything
 * bhrt_render_frame_ss_device refuses, as == NULL or as->enable_adaptive == 0, B < 1, M < B,
 * M > BHRT_SS_MAX_SAMPLES, width * height or either pass above INT_MAX rays (all of these before
 * any HIP call), or an allocation or HIP failure. */
int bhrt_render_frame_adaptive_device(const BlackHoleParams* blackhole,
                                      const AccretionDiskParams* disk,
                                      const SimulationConfig* config, const bhrt_camera* camera,
                                      int width, int height, const bhrt_rows* rows,
                                      IntegrationMethod method, int flags,
                                      const SupersamplingParams* ss,
                                      const AdaptiveSamplingParams* as,
                                      const bhrt_frame_soa* device_out, int32_t* device_samples,
                                      bhrt_adaptive_info* info, void* hip_stream);

/* The same whole frame into HOST arrays (host_samples may be NULL), on the current device;
 * returns when it is complete. */
int bhrt_render_frame_adaptive(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                               const SimulationConfig* config, const bhrt_camera* camera, int width,
                               int height, IntegrationMethod method, int flags,
                               const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                               const bhrt_frame_soa* host_out, int32_t* host_samples,
                               bhrt_adaptive_info* info);

/* ---- temporal accumulation: one jittered sample per pixel per frame, blended on the GPU ---- */

/* The visualizer's temporal path (TemporalAccumulationBuffer, renderer.h:39-48; accumulateFrame,
 * detectEdges, finalizeAccumulatedFrame, renderer.cpp:1759-1877) as an object on the device: every
 * frame is a plain camera frame at the next sub-pixel offset of a sample set, blended into a
 * running image. THE RULE -- all arithmetic is IEEE float32 with no contraction.
 * State of an accumulator of n pixels (a W x H image, or a bhrt_rows shard of it): acc[n][3] = 0,
 * edge[n] = 0, frame_count = 0, jitter_index = 0, reset_pending = 1. One step with a new frame
 * f[n][3]:
 *  1. if reset_pending: acc = 0, frame_count = 0, reset_pending = 0 (edge and jitter_index are
 *     kept, as resetAccumulation keeps them);
 *  2. alpha = bhrt_accum_alpha(params, frame_count): BHRT_ACCUM_REFERENCE 1.0f at frame_count 0,
 *     0.5f below 5, else blend_factor; BHRT_ACCUM_MEAN 1.0f / (float)(frame_count + 1), a running
 *     mean until max_frames caps frame_count and an exponential average from there;
 *  3. w = 1.0f - alpha (rounded once) and acc[i] = acc[i] * w + f[i] * alpha: two products and one
 *     sum. A NaN colour stays NaN until the next reset;
 *  4. frame_count = min(frame_count + 1, max_frames); jitter_index = (jitter_index + 1) % cycle;
 *  5. edges, whole images only, interior pixels 1..W-2 x 1..H-2, on the NEW acc: for the
 *     neighbours up, down, left and right d = (((0 + |dr|) + |dg|) + |db|) / 3.0f, g the largest d
 *     by `if (d > g) g = d` from 0 (a NaN d never raises it), and
 *     edge = g > edge_threshold ? 1.0f : max(0.0f, edge - edge_decay); border pixels stay 0;
 *  6. display rgba8: c' = max(0.0f, min(1.0f, c)) as std::max / std::min evaluate it (NaN -> 1),
 *     (unsigned char)(pow(c', 1.0f / 2.2f) * 255.0f) truncated toward zero, alpha byte 255, row 0 =
 *     the top image row. The power is the double pow of (double)c' and (double)(1.0f / 2.2f)
 *     rounded to float (the reference's float overload may differ from it by one byte step where
 *     the product lies within 255 * 16 * 2^-24 of an integer).
 * A rendered step takes f = (float) of the frame colour contract's rgb (what rgba32f holds) of the
 * plain camera frame whose offset is sample jitter_index (its value BEFORE step 4) of
 * bhrt_sample_offsets(ss, NULL), cycle = that call's count; ss == NULL or one sample: the pixel
 * centres every frame, cycle 1. Deviations from the reference: DESIGN.md section 14. */
typedef enum { BHRT_ACCUM_REFERENCE = 0, BHRT_ACCUM_MEAN = 1 } bhrt_accum_schedule;

typedef struct {
    int32_t schedule;        /* bhrt_accum_schedule                      default REFERENCE */
    float   blend_factor;    /* REFERENCE: alpha from frame_count 5 on            0.1f     */
    int32_t max_frames;      /* cap of frame_count                                32       */
    float   edge_threshold;  /* NaN: no edges                                     0.1f     */
    float   edge_decay;      /*                                                   0.2f     */
} bhrt_accum_params;         /* (initTemporalBuffer, renderer.cpp:1732-1739, :1842-1849)    */

typedef struct bhrt_accum bhrt_accum; /* opaque; owned by the thread and device that made it */

typedef struct {
    int32_t frame_count, jitter_index;
    int32_t reset_pending;   /* the next step starts from acc = 0                          */
    int32_t cycle;           /* count of bhrt_sample_offsets(ss, NULL) for bhrt_accum_info's ss */
    float   next_alpha;      /* the next step's alpha (1.0f where reset_pending)           */
    int32_t sharded;         /* a row shard: no edge factors                               */
    double  next_offset_x, next_offset_y; /* the next rendered step's sub-pixel offset     */
    int64_t frames_total;    /* steps since creation, resets not counted off               */
    int64_t pixels;          /* n                                                          */
} bhrt_accum_state;

typedef struct {             /* DEVICE buffers (HOST for bhrt_accum_frame); any may be NULL */
    uint8_t* rgba8;          /* [n][4] step 6                                              */
    float*   rgb;            /* [n][3] a copy of the new acc                               */
    float*   edge_factor;    /* [n] the new edge; whole images only                        */
} bhrt_accum_out;

/* Step 2's alpha for these parameters (NULL: the defaults) at this frame_count. Host only. */
float bhrt_accum_alpha(const bhrt_accum_params* params, int frame_count);

/* An accumulator for (the shard `rows` of) a width x height image on the CURRENT device: 28 B of
 * state and 16 B of frame scratch per pixel. params NULL: the defaults. Returns 0 and the handle
 * in *acc, or -1 with *acc untouched (bhrt_last_error): before any HIP call for a NULL acc, width
 * or height < 1, a bad row sharding, more than INT_MAX pixels, an unknown schedule, blend_factor
 * NaN or outside [0, 1], max_frames < 1, a negative or NaN edge_decay (a NaN edge_threshold is
 * valid: no edges); or an allocation or HIP failure. Waits for the device buffers' zero fill. */
int bhrt_accum_create(int width, int height, const bhrt_rows* rows, const bhrt_accum_params* params,
                      bhrt_accum** acc);

/* Frees the accumulator once the device has finished with it (waits for the device). NULL: no-op. */
void bhrt_accum_destroy(bhrt_accum* acc);

/* Sets reset_pending: what the viewer does on a camera or parameter change. 0, or -1 for NULL. */
int bhrt_accum_reset(bhrt_accum* acc);

/* The host-side state, with cycle and the next offset for `ss` (NULL: pixel centres). 0, or -1
 * (state untouched) for a NULL argument or a bhrt_sample_offsets refusal. No HIP call. */
int bhrt_accum_info(const bhrt_accum* acc, const SupersamplingParams* ss, bhrt_accum_state* state);

/* The accumulator's own device arrays, for zero-copy reading in stream order after a step:
 * *device_rgb = acc [n][3] float, *device_edge = edge [n] float (either pointer may be NULL). */
int bhrt_accum_device_buffers(const bhrt_accum* acc, const float** device_rgb,
                              const float** device_edge);

/* One rendered step: the plain camera frame at the next offset (the launch of
 * bhrt_render_frame_device with the offset in the camera, writing rgba32f into the accumulator's
 * scratch), then steps 1 to 6 in two small kernels, all on hip_stream. Asynchronous with NO host
 * wait: several frames can be in flight from one thread. NULL hip_stream is ordered like the legacy
 * default stream, exactly as for bhrt_render_frame_device. The host-side state (frame_count,
 * jitter_index, reset_pending, frames_total) advances AT THE CALL; the device work is stream-ordered.
 * The frames of one accumulator share its scratch frame and its state arrays, so THE CALLER ORDERS
 * THEM: the same stream for every step of an accumulator, or the caller's own events between the
 * streams it uses. bhrt_stats.rays gains n per frame; bhrt_set_claim_order applies as for the plain
 * frame. Returns 0, or -1 with nothing written and the state unchanged (bhrt_last_error), before
 * any HIP call for: a NULL acc, blackhole, config, camera or device_out; camera->use_offset != 0
 * (the accumulator sets the offsets); a bhrt_sample_offsets refusal (JITTER_RANDOM with more than
 * one sample, more than BHRT_SS_MAX_SAMPLES samples); device_out->edge_factor from a shard
 * accumulator; a current device other than the accumulator's; and for a HIP failure. */
int bhrt_accum_frame_device(bhrt_accum* acc, const BlackHoleParams* blackhole,
                            const AccretionDiskParams* disk, const SimulationConfig* config,
                            const bhrt_camera* camera, IntegrationMethod method, int flags,
                            const SupersamplingParams* ss, const bhrt_accum_out* device_out,
                            void* hip_stream);

/* accumulateFrame of the caller's own DEVICE frame device_rgb [n][3] float, then the same steps 4
 * to 6 with cycle = BHRT_SS_MAX_SAMPLES, the reference's literal 64 (a rendered step that finds
 * jitter_index at or above its own cycle takes it modulo that cycle first). Stream and state
 * rules as above; device_out may be NULL here (the state arrays alone are updated). */
int bhrt_accum_blend_device(bhrt_accum* acc, const float* device_rgb,
                            const bhrt_accum_out* device_out, void* hip_stream);

/* bhrt_accum_frame_device into HOST arrays, on the current device; returns when they are
 * complete. */
int bhrt_accum_frame(bhrt_accum* acc, const BlackHoleParams* blackhole,
                     const AccretionDiskParams* disk, const SimulationConfig* config,
                     const bhrt_camera* camera, IntegrationMethod method, int flags,
                     const SupersamplingParams* ss, const bhrt_accum_out* host_out);

/* Asynchronous form of bhrt_render_frame: queues the frame and returns a ticket (> 0) in
 * *ticket; the host arrays receive the frame through libbhrt's pinned staging (caller memory
 * is never page-locked) and must not be read or freed before bhrt_frame_wait(ticket) returns. Three
 * frames may be in flight per host thread; a fourth issue first completes the oldest frame,
 * whose own bhrt_frame_wait then returns its result (once). Each frame needs its own arrays. */
int bhrt_render_frame_async(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                            const SimulationConfig* config, const bhrt_camera* camera, int width,
                            int height, IntegrationMethod method, int flags,
                            const bhrt_frame_soa* host_out, int* ticket);

/* Wait for a frame queued by bhrt_render_frame_async; 0 when its host arrays are complete. */
int bhrt_frame_wait(int ticket);

/* Trace n rays already resident on the device (AoS Ray[n]) into DEVICE SoA buffers.
 * method RK4 with disk != NULL is trace_ray; RKF45 with a disk is integrate_photon_path
 * plus trace_ray's disk scan (config C3). hip_stream as for bhrt_render_frame_device (NULL:
 * ordered like the legacy default stream). */
int bhrt_trace_rays_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                           const AccretionDiskParams* disk, const SimulationConfig* config,
                           IntegrationMethod method, int flags,
                           const bhrt_frame_soa* device_out, void* hip_stream);

/* Host-buffer variant of the above (host Ray[n] in, host SoA out), multi-GPU split. */
int bhrt_trace_rays(const Ray* rays, int n, const BlackHoleParams* blackhole,
                    const AccretionDiskParams* disk, const SimulationConfig* config,
                    IntegrationMethod method, int flags, const bhrt_frame_soa* host_out);

/* ---- batched photon paths: the polylines of n rays in one launch ---- */
#define BHRT_PATHS_MAX_POSITIONS 65536

typedef struct {
    Vector3D* xyz;     /* [n][max_positions], ray-major: xyz + i*max_positions is ray i's polyline,
                          laid out as integrate_photon_path's own path_positions array          */
    float*    xyz32;   /* [n][max_positions][3], (float) of the same doubles: a GL vertex buffer  */
    int32_t*  count;   /* [n] points stored for ray i (<= max_positions)                          */
} bhrt_paths;          /* any pointer may be NULL: that output is not produced                    */

/* The recorded paths of n DEVICE rays into DEVICE arrays, asynchronous on hip_stream (NULL:
 * ordered like the legacy default stream, as for bhrt_trace_rays_device).
 * The full path q_0 .. q_{m-1} of ray i:
 *  - disk == NULL: what integrate_photon_path(origin with t = 0, direction, ..., method, ...)
 *    stores with max_positions unbounded (raytracer.c:504-507, 643-646): the origin, then one
 *    point per executed loop iteration -- the repeated points of a stuck RKF45 ray and of the
 *    "not implemented" LEAPFROG / YOSHIDA integrators included (max_integration_steps == 0: the
 *    origin alone);
 *  - disk != NULL: trace_ray's view of it (raytracer.c:717-759): if segment h is the first
 *    that hits the disk, q_0 .. q_{h-1} followed by the hit's hit_position (m = h + 1), else
 *    the full path.
 * every = e >= 1 keeps q_0, q_e, q_2e, ... and also q_{m-1} where (m - 1) % e != 0, so the end
 * of the ray is always drawn. Of that list the first max_positions points are stored (the
 * reference's own truncation) and count[i] is how many were; elements of xyz / xyz32 at or
 * beyond count[i] are NOT written. xyz32 holds (float) of xyz's doubles.
 * device_hits may be NULL; otherwise it receives what bhrt_trace_rays_device writes for the same
 * rays, disk, method and flags = 0 -- result, steps, hit_*, distance, time_dilation and sky_*,
 * bit for bit: the trace kernel's own launch, queued behind the path launch on the same stream
 * (the points are the single-ray path kernel's bits instead, so the last point of a long ray
 * and its hit_position may differ in their last digits); a non-NULL colour or display field is
 * an error.
 * Every element index into the path arrays is formed in size_t. bhrt_stats counts the path
 * launch as a trace launch (rays, iterations, launches), and the hits' launch as another.
 * Returns 0, or -1 with nothing written (bhrt_last_error): n <= 0; NULL device_rays, blackhole
 * or config; max_positions < 1 or > BHRT_PATHS_MAX_POSITIONS; every < 1; device_paths NULL or
 * all three of its pointers NULL; (long)n * max_positions > INT_MAX; a colour or display field
 * in device_hits; a HIP failure. */
int bhrt_trace_paths_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                            const AccretionDiskParams* disk, const SimulationConfig* config,
                            IntegrationMethod method, int max_positions, int every,
                            const bhrt_paths* device_paths, const bhrt_frame_soa* device_hits,
                            void* hip_stream);

/* The same with HOST arrays on the current device; returns when they are complete. Host
 * elements of xyz / xyz32 at or beyond count[i] keep what they held. */
int bhrt_trace_paths(const Ray* rays, int n, const BlackHoleParams* blackhole,
                     const AccretionDiskParams* disk, const SimulationConfig* config,
                     IntegrationMethod method, int max_positions, int every,
                     const bhrt_paths* host_paths, const bhrt_frame_soa* host_hits);

/* Diagnostic: both forms of the trace kernel's RKF45 accept test (the division-free fast
 * form and the reference's literal quotient, bhrt_trace_core.h rkf45_accept) on n cases of DEVICE
 * arrays err[6n], scale[6n], tol[n]; d_out[2i] / d_out[2i+1] = the two decisions. Returns 0
 * or a hipError_t value; asynchronous on hip_stream. */
int bhrt_check_rkf45_accept(const double* err, const double* scale, const double* tol, int n,
                            int* out, void* hip_stream);

/* Diagnostic: the trace loop's disk decision (bhrt_trace_core.h disk_hit) on n cases of DEVICE arrays
 * p[3n] (the point), d[3n] (the direction) and nrm[3n] (the plane "normal": the previous path
 * point), against the squared-radius thresholds in_sq <= s <= out_sq; d_out[i] = 1 for a hit.
 * Returns 0 or a hipError_t value; asynchronous on hip_stream. */
int bhrt_check_disk_hit(const double* p, const double* d, const double* nrm, int n, double in_sq,
                        double out_sq, int* out, void* hip_stream);

/* Diagnostic: the square root the trace loop takes for a segment's length (bhrt_trace_core.h
 * seg_len) of n DEVICE arguments x; d_out[i] = the root. Returns 0 or a hipError_t value;
 * asynchronous on hip_stream. */
int bhrt_check_seg_len(const double* x, int n, double* out, void* hip_stream);

/* Diagnostic: the reciprocal two RK4 a = 0 stages share (bhrt_trace_core.h pair_rcp) on n cases of a
 * DEVICE array in[4n] = (rc_a, st_a, rc_b, st_b), the stages' clamped r and sin theta;
 * d_out[5i..5i+3] = 1 / rc_a, 1 / st_a, 1 / rc_b, 1 / st_b as the stages form them, d_out[5i+4]
 * = 1.0 where the pair's range test passes (0.0: both stages take the literal form, not these).
 * huge != 0: with the rc < 1e150 test of the redo pass. Returns 0 or a hipError_t value;
 * asynchronous on hip_stream. */
int bhrt_check_pair_rcp(const double* in, int n, int huge, double* out, void* hip_stream);

/* Diagnostic: a chained angle shift of the RK4 a = 0 iteration (bhrt_trace_core.h shift_chain) on n
 * cases of a DEVICE array in[4n] = (a, s0, c0, x): sin and cos of x from s0 = sin a, c0 = cos a.
 * site 0: stage 3 from stage 2's angle (two coefficients, |x - a| <= 1/64); site 1: the advance
 * of state[1] from stage 4's angle (one coefficient, |x - a| <= 2^-10). d_out[5i..5i+1] = sin x,
 * cos x of the chained form, d_out[5i+2..5i+3] = those of shift_or_eval on the same operands,
 * d_out[5i+4] = 1.0 where the short polynomials were kept (0.0: the lane redid the shift with
 * shift_or_eval, and both pairs are equal bit for bit). Returns 0 or a hipError_t value
 * (hipErrorInvalidValue for another site); asynchronous on hip_stream. */
int bhrt_check_shift_chain(const double* in, int n, int site, double* out, void* hip_stream);

/* Diagnostic: a guard of the trace loop that is decided from the high words of its f64 operands
 * (bhrt_trace_core.h all_below_2), beside the exact test it filters for, on n cases of DEVICE
 * arrays. kind 0 (the one guard built): the plain-value test of a stage's three accelerations,
 * a[3n] (b is not read and may be NULL). d_out[2i] = 1 where the high-word filter keeps the case
 * on the straight-line path, d_out[2i+1] = 1 where the exact test (every |a| <= 10) passes; the
 * first implies the second. Returns 0 or a hipError_t value (hipErrorInvalidValue for another
 * kind); asynchronous on hip_stream. */
int bhrt_check_guard_words(const double* a, const double* b, int n, int kind, int* out,
                           void* hip_stream);

/* Copy and optionally reset this thread's statistics (waits for the timed launches, then reads
 * their counters with a synchronous copy on the legacy default stream, i.e. also after the
 * caller's default-stream work). out == NULL with reset != 0 drops the pending launches'
 * counters unread (no per-launch event timing): the cheap reset before a timed region. Returns
 * -1 if a launch whose redo pass was proved unnecessary handed a ray to it (bhrt_last_error). */
int bhrt_get_stats(bhrt_stats* out, int reset);

/* Number of GPUs libbhrt will use (HIP_VISIBLE_DEVICES / BHRT_MAX_DEVICES respected). */
int bhrt_device_count(void);

/* Tuning knob: refill a wavefront's finished lanes once at least this many are idle
 * (1..64; 0 = per scene: 8 for RK4 at spin 0, else 64). Affects speed only. */
void bhrt_set_refill_threshold(int lanes);

/* Tuning knob: the order in which this thread's next bhrt_render_frame_device calls of n rays
 * claim their rays -- d_order, an int array on the CURRENT device holding a permutation of
 * [0, n) (NULL or n = 0: the default order). Results are the same in any order; only the
 * schedule changes. The array is checked to be a permutation here (one D2H copy): returns 0,
 * or -1 (and the default order) if it is not. It applies only to device-API frames of exactly
 * n rays on the device that was current here, never to the chunks of bhrt_render_frame[_async]
 * host frames. libbhrt keeps the pointer: it must stay valid until the order is cleared
 * (bhrt_set_claim_order(NULL, 0)) or replaced. The check is a blocking copy on the legacy null
 * stream, which is NOT ordered after work on non-blocking streams (torch's, libbhrt's own):
 * synchronise the stream that wrote d_order before this call. The check costs a D2H copy, a
 * host sync and an O(n) scan per call; BHRT_TRUST_CLAIM_ORDER=1 skips it (the caller then
 * guarantees a permutation). Returns int since round 4 (void before). */
int bhrt_set_claim_order(const int* d_order, int n);

/* update_particles (particle_sim.c:505-566) applied `steps` times in one device round trip:
 * the particle array is copied to the GPU once, stepped `steps` times by the HIP kernel and
 * copied back (steps == 1 is exactly update_particles). Returns 0, or -1 on invalid
 * arguments / HIP failure. If kernel_ms is not NULL it receives the kernels' HIP-event time. */
int bhrt_update_particles_steps(ParticleSystem* system, const BlackHoleParams* blackhole,
                                const SimulationConfig* config, int steps, double* kernel_ms);

/* ---- device-resident particle systems: update and extract on the GPU ---- */

/* The visualizer's physics tick (bh_update_particles, then bh_get_particle_data into vertex
 * arrays, renderer.cpp:926-951, :1153-1219) on an object that keeps the Particle array on the
 * device: a tick is the update kernel and a few bytes per ACTIVE particle, no copy of the array.
 * update_particles, bhrt_update_particles_steps and the bh_* particle functions are unchanged.
 * THE RULE:
 *  State.    The object holds system->particles[0 .. count) on the device that was current at
 *            creation. create and upload copy the array in and WAIT for the copy. upload is for
 *            use after the caller changed the host system (add_particle, remove_particle); it may
 *            change count.
 *  Update.   bhrt_particles_update_device(ps, bh, cfg, s, stream) leaves the resident array in
 *            exactly the state bhrt_update_particles_steps(host_system, bh, cfg, s, NULL) leaves
 *            the host array in: every field of every particle bit for bit, the Inf/NaN of diverged
 *            test particles and the active flags of captured particles included; steps == 0 is a
 *            no-op. Asynchronous with NO host wait; `updates` advances AT THE CALL.
 *  Extract.  bh_get_particle_data on the resident array with *count = max_count: the first
 *            min(A, max_count) ACTIVE particles in array order, A the number of active particles.
 *            positions, velocities and types are copied, ids holds Particle.id, xyz32 and vel32 are
 *            (float) of the same doubles, count[0] is the number written. Elements at or beyond
 *            count[0] are NOT WRITTEN. The order is deterministic -- no atomic decides where a
 *            particle lands -- and the result is the same bits run to run and on any stream.
 *            bhrt_particles_extract does the same into HOST arrays and returns when they are
 *            complete; host elements beyond the count keep what they held.
 *  Download. Writes the resident particles into system->particles; refuses unless system->count
 *            equals the resident count; the system's other members are untouched. Waits for the
 *            copy.
 *  Streams.  hip_stream as for bhrt_render_frame_device: a stream is used as given, NULL is
 *            ordered like the legacy default stream. The calls of one object share its arrays, so
 *            THE CALLER ORDERS THEM, as for an accumulator: the same stream for every call on an
 *            object, or the caller's own events between the streams it uses. Objects are
 *            independent of each other. The calls that wait (upload, the host extract, download,
 *            destroy) first wait for the stream of the object's last update or device extract.
 *  Refusals. -1 with bhrt_last_error set, nothing written and no state changed, each decided
 *            BEFORE ANY HIP CALL: a NULL object, system, blackhole or config; system->count < 1 or
 *            NULL system->particles; steps < 0; max_count < 1; an output struct that is NULL or
 *            has all seven pointers NULL; a download count mismatch; a current device other than
 *            the object's. HIP failures also return -1. */
typedef struct bhrt_particles bhrt_particles;   /* opaque; owned by the thread and device that made it */

typedef struct {          /* DEVICE arrays (HOST for bhrt_particles_extract); any may be NULL      */
    double*  positions;   /* [max_count][3]  bh_get_particle_data's positions                      */
    double*  velocities;  /* [max_count][3]                                                        */
    int32_t* types;       /* [max_count]                                                           */
    int32_t* ids;         /* [max_count]     Particle.id                                           */
    float*   xyz32;       /* [max_count][3]  (float) of positions: a GL vertex buffer              */
    float*   vel32;       /* [max_count][3]  (float) of velocities                                 */
    int32_t* count;       /* [1]             particles written = min(active, max_count)            */
} bhrt_particle_data;

typedef struct { int32_t count, device; int64_t updates; } bhrt_particles_state;

/* A resident copy of system->particles[0 .. count) on the CURRENT device: 152 B per particle and
 * 8 B per 256 particles. Returns 0 and the handle in *ps, or -1 with *ps untouched. */
int  bhrt_particles_create(const ParticleSystem* system, bhrt_particles** ps);
/* The host system's array again (any count >= 1; the device buffer grows with slack). */
int  bhrt_particles_upload(bhrt_particles* ps, const ParticleSystem* system);
int  bhrt_particles_update_device(bhrt_particles* ps, const BlackHoleParams* blackhole,
                                  const SimulationConfig* config, int steps, void* hip_stream);
int  bhrt_particles_extract_device(bhrt_particles* ps, int max_count,
                                   const bhrt_particle_data* device_out, void* hip_stream);
int  bhrt_particles_extract(bhrt_particles* ps, int max_count, const bhrt_particle_data* host_out);
int  bhrt_particles_download(bhrt_particles* ps, ParticleSystem* system);
/* The resident array itself, for zero-copy reading in stream order (either pointer may be NULL). */
int  bhrt_particles_device_buffer(const bhrt_particles* ps, const Particle** device_particles,
                                  int* count);
/* The host-side state. No HIP call. */
int  bhrt_particles_info(const bhrt_particles* ps, bhrt_particles_state* state);
/* Frees the object once the device has finished with it (waits for the device). NULL: no-op. */
void bhrt_particles_destroy(bhrt_particles* ps);

/* A measurement aid (tools/bench_particles_resident.py): two update steps with the plain
 * kernel, two with the counting kernel (the second of each timed: both then follow an update pass
 * over the array), then the scan and the scatter of an extract into device_out, then the count pass
 * of create and upload, each between HIP events on libbhrt's own stream; waits, and returns the
 * five kernel times in ms[0..4]. The resident array advances by four steps (`updates` by 4).
 * Refusals as for the calls it makes. */
int  bhrt_particles_kernel_ms(bhrt_particles* ps, const BlackHoleParams* blackhole,
                              const SimulationConfig* config, int max_count,
                              const bhrt_particle_data* device_out, double ms[5]);

/* ---- Sky maps: an environment texture looked up where a ray leaves the scene ----
 * trace_pixel's two-colour background is a stand-in ("In a real implementation, this would be a
 * texture lookup", raytracer.c:1146-1157). With BHRT_FLAG_SKY a frame takes the colour of every
 * ray that is neither a disk hit nor a horizon ray from a caller's map instead.
 *
 * THE RULE (tests/sky_rule.py restates it in numpy).
 *  The map.    Equirectangular, W x H texels T[j][i][0..2] stored as float32. Row j = 0 touches
 *              theta = 0, the +z axis (the pole of cartesian_to_spherical, spacetime.c:201);
 *              column 0 starts at phi = -pi; texel centres lie at (i + 0.5, j + 0.5). Input formats:
 *              BHRT_SKY_RGB32F, [H][W][3] float; BHRT_SKY_RGBA8, [H][W][4] bytes, the texel
 *              (float)b / 255.0f, alpha ignored.
 *  The lookup  of a vector d, all of it IEEE double with no contraction:
 *              1. L = sqrt((dx dx + dy dy) + dz dz); a d whose L is not a finite value > 0 (a zero
 *                 or NaN vector, an overflowed sum) gives black, (0, 0, 0);
 *              2. theta = acos(clamp(dz / L, -1, 1));  3. phi = atan2(dy, dx);
 *              4. fx = (phi + pi) (W / (2 pi)) - 0.5, fy = theta (H / pi) - 0.5, the two factors
 *                 formed once, at bhrt_sky_create;
 *              5. i0 = floor(fx), wx = fx - i0, j0 = floor(fy), wy = fy - j0;
 *              6. columns wrap, i0 mod W and (i0 + 1) mod W; rows j0 and j0 + 1 clamp to [0, H - 1];
 *              7. c = (T00 (1 - wx) + T01 wx) (1 - wy) + (T10 (1 - wx) + T11 wx) wy per channel, on
 *                 (double) texels.
 *              Bilinear only: continuous across texel borders, the seam and the poles, so a
 *              last-digit difference in acos / atan2 moves the colour by a last digit. acos and
 *              atan2 are the device library's; the tests hold them to 1e-9 of the colour.
 *  Which d.    A RAY_MAX_DISTANCE ray -- the only class that has left the scene -- takes its EXIT
 *              CHORD d = p_k - p_(k-1), the two path points of the iteration that ended it (the
 *              last segment bhrt_trace_paths draws; RayTraceHit.sky_direction is unpinned for RK4
 *              and reads spherical components as Cartesian ones). A chord with a component that is
 *              not finite, or whose squared length (dx dx + dy dy) + dz dz is not > 0, does not
 *              count. That ray, and every other class but disk and horizon (RAY_MAX_STEPS: the
 *              step budget, a stuck RKF45 ray, max_integration_steps == 0, the no-op integrators),
 *              takes the direction the gradient reads: the ray's own initial direction.
 *              Disk and horizon colours are unchanged, and so is BHRT_FLAG_DOPPLER.
 *  The flag.   A frame uses the map only when flags has BHRT_FLAG_SKY AND a map is bound on the
 *              calling thread (bhrt_set_sky). The flag with no map bound returns -1. A bound map
 *              with no flag changes nothing: without the flag every call gives the bits it gave
 *              before. The flag travels with `flags` into every call that writes colour:
 *              bhrt_render_frame_device, bhrt_trace_rays_device and their host forms,
 *              bhrt_render_frame_ss*, bhrt_render_frame_adaptive*, bhrt_accum_frame*. The drop-in
 *              symbols have no flags argument and are unchanged.
 *  Devices.    A map lives on the device that was current at bhrt_sky_create. A call that would
 *              launch on another device returns -1 before any launch: the multi-GPU split of the
 *              host forms and bhrt_render_frame_gather included (one map per device is not
 *              offered).
 *  Refusals.   -1 with bhrt_last_error set and nothing written, each decided BEFORE ANY HIP CALL
 *              (the current device's query aside): a NULL argument; width or height < 1;
 *              width * height > 2^26; an unknown format; a float texel that is not finite; n < 1
 *              for the lookups; a current device other than the map's. HIP failures also return -1.
 *  Lifetime.   The map must outlive every frame queued with it; bhrt_sky_destroy waits for the
 *              device and unbinds the map if it is the calling thread's bound one. 16 bytes of
 *              device memory per texel (r, g, b and a pad: one tap is one aligned load). */
#define BHRT_SKY_RGB32F 0
#define BHRT_SKY_RGBA8  1
typedef struct bhrt_sky bhrt_sky;   /* opaque; owned by the thread and device that made it */
typedef struct { int32_t width, height, format, device; } bhrt_sky_state;

/* A map of host_texels on the CURRENT device, complete on return. 0 and the handle in *sky, or -1
 * with *sky untouched. */
int  bhrt_sky_create(const void* host_texels, int width, int height, int format, bhrt_sky** sky);
/* Waits for the device, unbinds the map if it is bound on this thread, frees it. NULL: no-op. */
void bhrt_sky_destroy(bhrt_sky* sky);
/* width, height, format, device. No HIP call. */
int  bhrt_sky_info(const bhrt_sky* sky, bhrt_sky_state* state);
/* The calling thread's map for frames with BHRT_FLAG_SKY; NULL unbinds. No HIP call. */
int  bhrt_set_sky(const bhrt_sky* sky);
/* The lookup alone: device_rgb[i] = the lookup of device_dirs[i], n >= 1 packed vectors, queued
 * on hip_stream (NULL: ordered like the legacy default stream), no host wait. */
int  bhrt_sky_lookup_device(const bhrt_sky* sky, const double* device_dirs /* [n][3] */, int n,
                            double* device_rgb /* [n][3] */, void* hip_stream);
/* The same on host arrays; waits. */
int  bhrt_sky_lookup(const bhrt_sky* sky, const double* dirs, int n, double* rgb);

/* ---- Physical geodesics: a Kerr-Schild null-ray tracer beside the parity path ----
 * The calls above reproduce the reference ray for ray: with spin != 0 its accelerations are zero
 * ("Kerr geodesic equations would go here", raytracer.c:131-138) and every ray is a straight line;
 * with spin == 0 the state is read index-shifted and clamped. The bhrt_kerr_* calls trace true null
 * geodesics of Kerr (Schwarzschild is spin 0) instead: an opt-in path with its own kernel, which
 * changes nothing in the calls above.
 *
 * THE RULE (tests/kerr_rule.py restates it in numpy). All arithmetic is IEEE double.
 *  Time reversal. The ray of image direction n is the time reverse of the photon that arrives from
 *              n, and time reversal maps Kerr(a) onto Kerr(-a): the kernel integrates a
 *              future-directed photon that leaves the origin along n, in ingoing Kerr-Schild
 *              coordinates of spin a~ = -(spin * mass). Rays cross the future horizon smoothly; for
 *              spin > 0 about +z the flat prograde edge of the shadow lies on the side of the image
 *              where the hole turns toward the observer. All positions -- origins, hit points,
 *              chords, the disk -- are Kerr-Schild Cartesian coordinates: at spin 0 the project's
 *              spherical identification, far from the hole flat space.
 *  Geometry    at (x, y, z): rho^2 = x^2 + y^2 + z^2, w = rho^2 - a~^2, D = sqrt(w^2 + 4 a~^2 z^2),
 *              r^2 = (w + D) / 2, r = sqrt(r^2), G = r^4 + a~^2 z^2, S = r^2 + a~^2,
 *              f = 2 M r^3 / G, l = ((r x + a~ y) / S, (r y - a~ x) / S, z / r).
 *  Hamiltonian H = 1/2 [-E^2 + p.p - f u^2] with u = E + l.p; E > 0 is constant along the ray.
 *  Equations   xdot_i = p_i - f u l_i, pdot_i = 1/2 (d_i f) u^2 + f u (d_i l_j) p_j, with the
 *              analytic gradients dr = (x r / D, y r / D, z S / (r D)),
 *              d_i f = f (3 d_i r / r - (4 r^3 d_i r + 2 a~^2 z delta_iz) / G),
 *              d_i l_x = (x d_i r + r delta_ix + a~ delta_iy) / S - l_x 2 r d_i r / S,
 *              d_i l_y = (y d_i r + r delta_iy - a~ delta_ix) / S - l_y 2 r d_i r / S,
 *              d_i l_z = delta_iz / r - z d_i r / r^2.
 *  Initial data. A static observer at the origin with local photon energy 1 and unit direction n
 *              (a ray's direction is normalised, n = d / sqrt((dx^2 + dy^2) + dz^2), and so is a
 *              camera pixel's -- calculate_ray_direction's unit vector, formed with one operation
 *              per rounding, goes through the same division again):
 *              kappa = sqrt(1 - f), v = n + (kappa - 1)(l.n) l, k^t = 1 / kappa + f (l.v) / (1 - f),
 *              p = v + f (k^t + l.v) l, E = kappa; H = 0 holds by construction. An origin with
 *              f >= 1 or r <= r+ has no static observer: the camera and host-ray calls refuse it
 *              before any HIP call, a device ray there gets RAY_ERROR with steps 0.
 *  Step.       Classical RK4 on (x, p); h = time_step min(1, max(r / (8 M), 1 / 16)), r at the
 *              step's start.
 *  After each step, in this order, with p_old, p_new the two points, c = p_new - p_old and
 *              seg = sqrt((cx^2 + cy^2) + cz^2):
 *              1. any non-finite state component: RAY_ERROR;
 *              2. with a disk: a crossing is (z_old > 0 and z_new <= 0) or (z_old < 0 and
 *                 z_new >= 0); then t = z_old / (z_old - z_new), q = p_old + t c, a hit iff
 *                 in^2 + a~^2 <= q_x^2 + q_y^2 <= out^2 + a~^2 (Boyer-Lindquist radius in [in, out]
 *                 on the equator; both bounds formed once on the host): RAY_DISK, hit = (q_x, q_y,
 *                 0), distance += t seg. The first hit wins;
 *              3. r_new <= r+ = M + sqrt(M^2 - a~^2): RAY_HORIZON;
 *              4. distance += seg; distance > max_ray_distance: RAY_MAX_DISTANCE;
 *              5. steps >= max_integration_steps: RAY_MAX_STEPS (max_integration_steps == 0: at the
 *                 origin, with steps 0).
 *  Outputs     (bhrt_frame_soa): result; steps, the number of RK4 steps; hit_*, the last point or
 *              the disk point; distance; sky_*, the exit chord c of a RAY_MAX_DISTANCE ray (other
 *              rays' elements are not written); time_dilation must be NULL.
 *  Colour.     The frame colour contract: the disk colour of (hit_x, hit_y),
 *              BHRT_FLAG_DOPPLER reading the hitting segment's unit chord as d; black for the
 *              horizon; every other ray the gradient, read on the unit EXIT CHORD's y if it is
 *              RAY_MAX_DISTANCE -- which is what shows the lensing in the background -- else on n's
 *              y. With BHRT_FLAG_SKY the sky-map rule applies unchanged (chord lookup, else n).
 *  Determinism. No atomic in any output: a ray's outputs are a pure function of its inputs, the
 *              same bits run to run, on any stream, in any row-shard split, and through the camera
 *              and the ray-array entry points (one kernel instantiation serves them all).
 *  Diagnostics (bhrt_kerr_diag, optional per-ray arrays, device or host as the call's outputs):
 *              h_residual, the largest |(-E^2 + p.p - f u^2) / (E^2 + p.p + f u^2)| over the ray's
 *              accepted points (the origin and every finite step end); lz_drift,
 *              |(x p_y - y p_x)_end - (x p_y - y p_x)_0| at the last finite step end.
 *  Refusals.   -1 with bhrt_last_error set and nothing written, each decided BEFORE ANY HIP CALL
 *              (the current device's query aside): a NULL blackhole, config or output struct;
 *              |spin| >= 1 or NaN; mass not finite or not > 0; time_step not finite or not > 0;
 *              max_integration_steps < 0; a NaN max_ray_distance; a disk with NaN or negative
 *              radii; time_dilation != NULL; rgb not given as all three channels; an origin
 *              without a static observer (camera and host-ray calls); n <= 0, width or height < 1,
 *              a bad row sharding; BHRT_FLAG_SKY without a map bound on this device. HIP failures
 *              also return -1.
 *  Statistics. bhrt_stats counts a launch as a trace launch: rays, iterations (RK4 steps), launches.
 *  Not offered. The supersampled, adaptive and accumulator calls do not take this path; a caller
 *              accumulates these frames through bhrt_accum_blend_device. Recorded polylines of
 *              these rays: "Physical photon paths" below. */
typedef struct {
    double* h_residual;
    double* lz_drift;
} bhrt_kerr_diag;

/* (A shard of) a camera frame into DEVICE arrays on hip_stream: asynchronous, no host wait; NULL
 * is ordered like the legacy default stream, as for bhrt_render_frame_device. camera->use_offset
 * and row shards are honoured. diag may be NULL. */
int bhrt_kerr_frame_device(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                           const SimulationConfig* config, const bhrt_camera* camera, int width,
                           int height, const bhrt_rows* rows, int flags,
                           const bhrt_frame_soa* device_out, const bhrt_kerr_diag* device_diag,
                           void* hip_stream);
/* The whole frame into HOST arrays on the current device; returns when they are complete. */
int bhrt_kerr_frame(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                    const SimulationConfig* config, const bhrt_camera* camera, int width, int height,
                    int flags, const bhrt_frame_soa* host_out, const bhrt_kerr_diag* host_diag);
/* n DEVICE rays (AoS Ray[n]) into DEVICE arrays, stream as above. */
int bhrt_kerr_rays_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                          const AccretionDiskParams* disk, const SimulationConfig* config, int flags,
                          const bhrt_frame_soa* device_out, const bhrt_kerr_diag* device_diag,
                          void* hip_stream);
/* n HOST rays into HOST arrays on the current device; returns when they are complete. */
int bhrt_kerr_rays(const Ray* rays, int n, const BlackHoleParams* blackhole,
                   const AccretionDiskParams* disk, const SimulationConfig* config, int flags,
                   const bhrt_frame_soa* host_out, const bhrt_kerr_diag* host_diag);
/* The initial data of one ray on the host, with the device's operations: state = (x, p), *E = E.
 * 0, or -1 (nothing written) for a NULL argument, a bad blackhole as above, or an origin without
 * a static observer. No HIP call. */
int bhrt_kerr_ray_init(const BlackHoleParams* blackhole, const Vector3D* origin,
                       const Vector3D* direction, double state[6], double* E);

/* ---- Physical geodesics, adaptive steps: Dormand-Prince 5(4) under config->tolerance ----
 * The calls above have one accuracy knob, time_step, pin the step at time_step beyond 8 M and
 * ignore config->tolerance. The bhrt_kerr_rk45_* calls trace the same rays with an embedded pair
 * and a step chosen by tolerance: long steps in nearly flat space, short ones near the hole, and a
 * disk point on the step's cubic instead of its chord. An opt-in path with its own kernel; every
 * call above keeps its bits.
 *
 * THE ADAPTIVE RULE (tests/kerr_rk45_rule.py restates it in numpy). Time reversal, geometry,
 * Hamiltonian, equations, initial data and the observer refusal are those of THE RULE above,
 * unchanged; y = (x, p) is the six-component state and ydot its derivative.
 *  Pair.       Dormand-Prince 5(4): the standard 7-stage tableau with FSAL (c = 0, 1/5, 3/10, 4/5,
 *              8/9, 1, 1). The new point ynew is the 5th-order solution, stage 7 is ydot(ynew), and
 *              the error vector is e = h sum_j (b5_j - b4_j) k_j. An accepted attempt's k7 is the
 *              next attempt's k1; a rejected attempt keeps its k1. Sums run over the non-zero
 *              weights from j = 1 up, left to right.
 *  Trial step. h_try = min(h, r / 2) with r at the attempt's start, so no attempt leaps the hole;
 *              the first h is time_step.
 *  Error norm. sc_c = tol (1 + max(|y_c|, |ynew_c|)) over the six components,
 *              err = max_c |e_c| / sc_c, tol = config->tolerance.
 *  Controller. fac = min(5, max(0.2, 0.9 err^(-1/5))), a non-finite fac is 0.2; h = h_try fac
 *              after an accepted and after a rejected attempt alike. Accepted iff err <= 1. Every
 *              attempt counts: steps is the number of attempts, rejected[i] those not accepted.
 *  After each attempt, in this order, with seg = |x_new - x_old|:
 *              1. a non-finite ynew or err: RAY_ERROR, the ray ends on that point;
 *              2. after a rejection the state stays and only test 6 runs;
 *              3. with a disk: the crossing test on z_old, z_new is THE RULE's. The crossing is
 *                 located on the cubic Hermite polynomial of z through the two end points with end
 *                 derivatives h_try k1_z and h_try k7_z: q(theta) = q_old + theta (m0 + theta (c2
 *                 + theta c3)), d = q_new - q_old, c2 = (3 d - 2 m0) - m1, c3 = (m0 + m1) - 2 d.
 *                 theta = z_old / (z_old - z_new), then four Newton iterations
 *                 theta = clamp(theta - z(theta) / z'(theta), 0, 1), a non-finite iterate keeping
 *                 theta. q_x, q_y are the Hermite polynomials of x, y at theta; the hit test on
 *                 q_x^2 + q_y^2 is THE RULE's: RAY_DISK, hit = (q_x, q_y, 0),
 *                 distance += theta seg. The first hit wins;
 *              4. r_new <= r+: RAY_HORIZON;
 *              5. distance += seg; distance > max_ray_distance: RAY_MAX_DISTANCE;
 *              6. attempts >= max_integration_steps: RAY_MAX_STEPS (max_integration_steps == 0: at
 *                 the origin, with steps 0).
 *  Outputs     are THE RULE's with two differences: sky_* of a RAY_MAX_DISTANCE ray is the EXIT
 *              TANGENT, xdot at the end point (the FSAL stage's first three components), not the
 *              chord -- adaptive steps are long, and a chord is not the exit direction; and the
 *              Doppler direction of a disk hit is the unit Hermite derivative of position at theta.
 *              Colour, the sky-map rule, rgba32f / rgba8 and determinism follow the text above with
 *              "chord" read as this tangent.
 *  Diagnostics (bhrt_kerr_rk45_diag): h_residual and lz_drift as above, taken over accepted points
 *              only (the origin and every accepted ynew); rejected, int per ray.
 *  Refusals.   Those above, each decided BEFORE ANY HIP CALL, and one more: config->tolerance must
 *              be finite and within [1e-12, 1e-2] (below 1e-12 the error estimate is rounding
 *              noise). time_step keeps its checks and becomes the first trial step.
 *  Statistics. One trace launch; iterations counts attempts.
 *  Not offered. Recorded paths of these rays: bhrt_kerr_paths* stays RK4. */
typedef struct {
    double* h_residual;
    double* lz_drift;
    int* rejected;
} bhrt_kerr_rk45_diag;

/* The four calls of "Physical geodesics" in argument types and order, stream rule included. */
int bhrt_kerr_rk45_frame_device(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                                const SimulationConfig* config, const bhrt_camera* camera,
                                int width, int height, const bhrt_rows* rows, int flags,
                                const bhrt_frame_soa* device_out,
                                const bhrt_kerr_rk45_diag* device_diag, void* hip_stream);
int bhrt_kerr_rk45_frame(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                         const SimulationConfig* config, const bhrt_camera* camera, int width,
                         int height, int flags, const bhrt_frame_soa* host_out,
                         const bhrt_kerr_rk45_diag* host_diag);
int bhrt_kerr_rk45_rays_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                               const AccretionDiskParams* disk, const SimulationConfig* config,
                               int flags, const bhrt_frame_soa* device_out,
                               const bhrt_kerr_rk45_diag* device_diag, void* hip_stream);
int bhrt_kerr_rk45_rays(const Ray* rays, int n, const BlackHoleParams* blackhole,
                        const AccretionDiskParams* disk, const SimulationConfig* config, int flags,
                        const bhrt_frame_soa* host_out, const bhrt_kerr_rk45_diag* host_diag);

/* ---- Physical photon paths: batched polylines of true Kerr geodesics ----
 * bhrt_trace_paths records the parity path's rays, straight lines wherever spin != 0. These calls
 * record the rays of "Physical geodesics" above instead -- how light bends: the lensing diagram,
 * the orbits that wind round the photon sphere, the prograde / retrograde asymmetry behind the
 * D-shaped shadow -- n rays in one launch, into bhrt_paths arrays laid out as bhrt_trace_paths'.
 *
 * THE RULE (tests/kerr_paths_rule.py restates it in numpy).
 *  Full path   of ray i: q_0 .. q_{m-1} with m = steps + 1, steps being the Physical-geodesics
 *              rule's step count for that ray, disk, config and spin. q_0 is the ray's origin as
 *              given; q_k (1 <= k <= steps) is the position the rule keeps after step k: the step's
 *              end point, except that the disk-hitting step contributes the hit point
 *              (q_x, q_y, 0). So a RAY_DISK path ends on the disk, a RAY_HORIZON path on its first
 *              point with r <= r+, a RAY_MAX_DISTANCE path on the first point past the distance, a
 *              RAY_MAX_STEPS path on point max_integration_steps, and a RAY_ERROR from a non-finite
 *              state on that non-finite point, stored as it is: q_{m-1} is always what hit_x/y/z
 *              holds. A device ray whose origin has no static observer has m = 1, the origin alone,
 *              and so has every ray with max_integration_steps == 0.
 *  Stored points (bhrt_trace_paths_device's rule, word for word). every = e >= 1 keeps q_0, q_e,
 *              q_2e, ... and also q_{m-1} where (m - 1) % e != 0, so the end of the ray is always
 *              drawn. Of that list the first max_positions points are stored and count[i] is how
 *              many were; elements of xyz / xyz32 at or beyond count[i] are NOT written. xyz32
 *              holds (float) of xyz's doubles. Every element index into the path arrays is formed
 *              in size_t.
 *  Hit records. device_hits may be NULL; otherwise it and device_diag receive exactly what
 *              bhrt_kerr_rays_device(device_rays, n, blackhole, disk, config, flags, device_hits,
 *              device_diag, hip_stream) writes, bit for bit: that call's own k_kerr launch, queued
 *              behind the path launch on the same stream. Colour fields and BHRT_FLAG_SKY are
 *              allowed, so a caller can draw each path in its pixel's colour; flags is not
 *              otherwise used. device_diag without device_hits is refused.
 *  Which bits. The points come from the path kernel and the records from k_kerr: two compilations
 *              of one step. q_{m-1} and hit_* agree to 1e-5 of the larger magnitude (the GPU
 *              suite's contract), not necessarily in every bit; count[i] is the path kernel's own,
 *              and so is the class it implies.
 *  Determinism. No atomic touches an output: a ray's row is a pure function of its own inputs, the
 *              same bits run to run, on any stream, whatever n is and wherever the ray stands in
 *              the batch.
 *  Statistics. bhrt_stats counts the path launch as a trace launch (rays n, iterations the sum of
 *              steps, launches 1) and the hit records' launch as another.
 *  Refusals.   -1 with bhrt_last_error set, nothing written and nothing launched, each decided
 *              BEFORE ANY HIP CALL (the current device's query aside), the path arguments and the
 *              hit arguments alike before the first launch: everything bhrt_kerr_rays_device
 *              refuses for the scene (|spin| >= 1 or NaN; mass; time_step; max_integration_steps
 *              < 0; a NaN max_ray_distance; disk radii) and for device_hits (time_dilation != NULL;
 *              rgb not given as all three channels; BHRT_FLAG_SKY without a map bound on this
 *              device); n <= 0; NULL rays, blackhole or config; max_positions < 1 or
 *              > BHRT_PATHS_MAX_POSITIONS; every < 1; device_paths NULL or all three of its
 *              pointers NULL; (long)n * max_positions > INT_MAX; device_diag without device_hits;
 *              in the host form only, an origin without a static observer (as bhrt_kerr_rays). HIP
 *              failures also return -1.
 * Asynchronous on hip_stream, no host wait; NULL is ordered like the legacy default stream, as for
 * bhrt_render_frame_device. */
int bhrt_kerr_paths_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                           const AccretionDiskParams* disk, const SimulationConfig* config,
                           int max_positions, int every, int flags,
                           const bhrt_paths* device_paths, const bhrt_frame_soa* device_hits,
                           const bhrt_kerr_diag* device_diag, void* hip_stream);
/* The same with HOST arrays on the current device; returns when they are complete. Host elements
 * of xyz / xyz32 at or beyond count[i] keep what they held. */
int bhrt_kerr_paths(const Ray* rays, int n, const BlackHoleParams* blackhole,
                    const AccretionDiskParams* disk, const SimulationConfig* config,
                    int max_positions, int every, int flags, const bhrt_paths* host_paths,
                    const bhrt_frame_soa* host_hits, const bhrt_kerr_diag* host_diag);

/* ---- Kerr disk emission: the redshift factor and higher-order disk images ----
 * The calls above colour a disk pixel by the frame colour contract -- with BHRT_FLAG_DOPPLER the
 * reference's stand-in, not a redshift -- and end every ray at its first disk crossing. The
 * bhrt_kerr_emit_* calls give what a line-profile or EHT-style image code starts from: the
 * frequency ratio g = E_obs / E_emit of every disk crossing, the bolometric intensity g^4 eps(r)
 * built from it, and the disk's higher-order images (the secondary image under the shadow, the
 * photon ring). An opt-in path with its own kernel; every call above keeps its bits.
 *
 * THE EMISSION RULE (tests/kerr_emit_rule.py restates it in numpy). Everything is THE ADAPTIVE RULE
 * above -- initial data, attempts, controller, the order of the tests, the Hermite crossing point,
 * the exit tangent -- with these differences.
 *  Crossings.  A crossing is what test 3 finds: an accepted attempt whose Hermite point has
 *              q_x^2 + q_y^2 within [in^2 + a~^2, out^2 + a~^2]. Crossing number k (0-based) of a ray
 *              is recorded. K = max_crossings, 1 <= K <= BHRT_EMIT_MAX_CROSSINGS. If k + 1 < K the
 *              ray continues from the attempt's end point ynew unchanged: distance += seg, k1 = k7,
 *              and tests 4 to 6 run as after any accepted attempt. If k + 1 == K the ray ends as the
 *              adaptive rule ends it: RAY_DISK, hit = (q_x, q_y, 0), distance += theta seg. One
 *              attempt holds at most one crossing (the sign test on z_old, z_new). With K = 1 the
 *              bhrt_frame_soa hit fields, steps and rejected are the adaptive rule's.
 *  Redshift    of a crossing, with a = spin * mass (the physical spin, not a~; a^2 = a~^2),
 *              s2 = q_x^2 + q_y^2 and M = mass: r = sqrt(s2 - a^2);
 *              Omega = sqrt(M) / (r sqrt(r) + a sqrt(M)), the disk turning about +z in +phi as the
 *              Doppler term above assumes;
 *              N = (1 - (2M / r)(1 - a Omega)^2) - Omega^2 (r^2 + a^2), which is
 *              -g_mu_nu u^mu u^nu / (u^t)^2 of u ~ d_t + Omega d_phi read off the Kerr-Schild metric
 *              on the equator; g = sqrt(N) / (E + Omega L_z) with E and L_z = x p_y - y p_x of the
 *              initial data, constants of the motion (the integrated photon is the time reverse of
 *              the observed one, so the disk's angular velocity enters as -Omega: hence the plus
 *              sign). g = 0 where N > 0 or E + Omega L_z > 0 fails or g is not finite: no circular
 *              orbit there. bhrt_kerr_disk_redshift is this arithmetic on the host.
 *  Emission.   eps(r) = pow(inner_radius / r, emissivity_index); w_k = (g_k^2)^2 eps(r_k);
 *              intensity = sum_k w_k over the recorded crossings in order (optically and
 *              geometrically thin), 0 for a ray without crossings.
 *  Outputs     (bhrt_kerr_emit_out; every pointer optional): count[n], int; radius[K][n] and
 *              redshift[K][n], plane-major, the element index k n + i formed in size_t;
 *              intensity[n]. Elements of radius and redshift with k >= count[i] are NOT written. The
 *              bhrt_frame_soa fields keep their adaptive-rule meaning: hit_* is the last point, or
 *              the K-th crossing. At least one output overall, of either struct.
 *  Colour.     A ray with count 0 gets the adaptive rule's colour: horizon black, otherwise the
 *              gradient on the exit tangent or n, the sky-map rule under BHRT_FLAG_SKY. A ray with
 *              crossings gets per channel clamp(gain sum_k w_k base_k, 0, 1), base_k the frame
 *              colour contract's disk colour at (q_x, q_y) of crossing k without the Doppler block.
 *              BHRT_FLAG_DOPPLER is refused: g replaces it.
 *  Refusals.   Each decided BEFORE ANY HIP CALL, -1 with bhrt_last_error set and nothing written:
 *              everything bhrt_kerr_rk45_* refuses; a NULL disk; a NULL params; max_crossings
 *              outside 1..BHRT_EMIT_MAX_CROSSINGS; emissivity_index or gain not finite or < 0;
 *              BHRT_FLAG_DOPPLER; no output at all; (long)K * n > INT_MAX.
 *  Determinism, statistics, streams. As for the adaptive calls: no atomic in any output, one trace
 *              launch, iterations counts attempts, a NULL hip_stream is ordered like the legacy
 *              default stream. The diagnostics are bhrt_kerr_rk45_diag's.
 *  Not offered. Limb darkening, a Novikov-Thorne flux, emission inside the ISCO's plunging region
 *              beyond g = 0, emission on the fixed-step calls or the path recorder. */
#define BHRT_EMIT_MAX_CROSSINGS 4
typedef struct {
    int max_crossings;
    double emissivity_index;
    double gain;
} bhrt_kerr_emit_params;

typedef struct {
    int* count;
    double* radius;
    double* redshift;
    double* intensity;
} bhrt_kerr_emit_out;

/* The four calls of "Physical geodesics, adaptive steps" with the emission's parameters and outputs
 * (device or host arrays, as the call's other outputs; emit_out may be NULL). */
int bhrt_kerr_emit_frame_device(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                                const SimulationConfig* config, const bhrt_camera* camera,
                                int width, int height, const bhrt_rows* rows, int flags,
                                const bhrt_frame_soa* device_out,
                                const bhrt_kerr_rk45_diag* device_diag,
                                const bhrt_kerr_emit_params* params,
                                const bhrt_kerr_emit_out* device_emit, void* hip_stream);
int bhrt_kerr_emit_frame(const BlackHoleParams* blackhole, const AccretionDiskParams* disk,
                         const SimulationConfig* config, const bhrt_camera* camera, int width,
                         int height, int flags, const bhrt_frame_soa* host_out,
                         const bhrt_kerr_rk45_diag* host_diag,
                         const bhrt_kerr_emit_params* params, const bhrt_kerr_emit_out* host_emit);
int bhrt_kerr_emit_rays_device(const Ray* device_rays, int n, const BlackHoleParams* blackhole,
                               const AccretionDiskParams* disk, const SimulationConfig* config,
                               int flags, const bhrt_frame_soa* device_out,
                               const bhrt_kerr_rk45_diag* device_diag,
                               const bhrt_kerr_emit_params* params,
                               const bhrt_kerr_emit_out* device_emit, void* hip_stream);
int bhrt_kerr_emit_rays(const Ray* rays, int n, const BlackHoleParams* blackhole,
                        const AccretionDiskParams* disk, const SimulationConfig* config, int flags,
                        const bhrt_frame_soa* host_out, const bhrt_kerr_rk45_diag* host_diag,
                        const bhrt_kerr_emit_params* params, const bhrt_kerr_emit_out* host_emit);
/* g of the Redshift paragraph for a crossing at Boyer-Lindquist radius `radius` of a photon with
 * constants E and lz, on the host with the device's operations. 0 and *g, or -1 (nothing written)
 * for a NULL argument or a bad blackhole as above. No HIP call. */
int bhrt_kerr_disk_redshift(const BlackHoleParams* blackhole, double radius, double E, double lz,
                            double* g);

/* ---- Physical particles: timelike geodesics for resident systems ----
 * bhrt_particles_update_device reproduces the reference's update_particles operation for
 * operation: an Euler step on a four-entry subset of the Christoffel symbols for a test particle
 * inside 20 rs, Newtonian gravity for every other. No orbit of it is stable, nothing knows the ISCO
 * and nothing plunges. bhrt_particles_kerr_update_device advances the same resident object along
 * true timelike geodesics of Kerr in coordinate time instead: an opt-in update with its own kernel,
 * beside the parity update; every call above keeps its bits.
 *
 * THE PARTICLE RULE (tests/kerr_particles_rule.py restates it in numpy). All arithmetic is IEEE
 * double.
 *  Spin.       a = +(spin * mass), not a~: particles run forward in time, so there is no time
 *              reversal. Geometry, Hamiltonian and Equations are THE RULE's of "Physical geodesics"
 *              with a~ replaced by a. With this sign the disk's prograde circular orbits (about +z
 *              in +phi, bhrt_kerr_orbit_velocity) are circular; with the other they plunge.
 *  State.      position is Kerr-Schild Cartesian; velocity is the coordinate velocity dx/dt against
 *              Kerr-Schild time t, which is what a tick advances: all particles of a system stay on
 *              one time slice.
 *  From velocity to momentum, at the start of every call, per active particle, with f and l at x
 *              and unit rest mass (Particle.mass is not read): w = 1 + l.v,
 *              N = (1 - v.v) - f w^2; the particle is timelike iff N is finite and > 0;
 *              u^t = 1 / sqrt(N), p = u^t (v + f w l), E = u^t (1 - f w), L_z = x p_y - y p_x.
 *              H = -1/2 holds by construction.
 *  Equations.  xdot and pdot as for the rays; tdot = E + f u with u = E + l.p. Integrated against
 *              t: d(x, p)/dt = (xdot, pdot) / tdot and dtau/dt = 1 / tdot, seven components, the
 *              reciprocal of tdot formed once per stage.
 *  Tick.       One tick advances t by dt = config->time_step. With r at the tick's start,
 *              m = substeps ceil(1 / min(1, max(r / (8 M), 1 / 16))) -- the ray rule's step schedule
 *              as an integer count -- and h = dt / m. A tick is m classical RK4 steps of size h on
 *              the seven components, with the ray rule's weights and summation order. A tick that
 *              begins adds dt to age and to coordinate_time.
 *  After each substep, in this order:
 *              1. any non-finite component: the particle keeps the state it had before that
 *                 substep, active = 0, status ERROR, and the call is over for it;
 *              2. r_new <= r+ = M + sqrt(M^2 - a^2): captured, active = 0, status CAPTURED, the
 *                 position is that point, and the call is over for it. Ingoing Kerr-Schild
 *                 coordinates are regular on the horizon: a plunging particle arrives there with
 *                 finite fields.
 *  At the call's start, nothing else being written in each case: a particle with active == 0 is
 *              not touched, in any byte; an active particle with r <= r+ is captured, active = 0 and
 *              status CAPTURED (decided first, whatever its velocity); an active particle that is
 *              not timelike gets status NOT_TIMELIKE, is not touched and stays active.
 *  Written at the end, for a particle that ran: position; velocity = xdot / tdot at the last point;
 *              energy = E; angular_momentum = x p_y - y p_x at the last point; proper_time += the
 *              tau integrated in this call; coordinate_time; age; time_dilation = tdot at the last
 *              point (dt/dtau, >= 1 far away); active. acceleration, mass, type, id and temperature
 *              keep their bytes. Every ParticleType moves by the same rule.
 *  Block counts. The launch leaves the object's per-256-particle active counts as the parity
 *              update leaves them, counted after the update: bhrt_particles_extract* works
 *              unchanged after either kind of update. updates advances by one per call, AT THE CALL.
 *  Composition. E is formed again from velocity at every call: two calls of s ticks agree with one
 *              call of 2 s ticks to rounding in position and velocity, NOT IN BITS; energy,
 *              angular_momentum, time_dilation and the later proper_time agree to half the
 *              |2H + 1| that the integrator left on the state carried up to the split.
 *  Determinism. No atomic touches an output: a particle's result is a pure function of its own
 *              fields and the scene, the same bits run to run, on any stream, whatever the count
 *              and wherever the particle stands in the array.
 *  Diagnostics (bhrt_kerr_particles_diag, optional DEVICE arrays [count] by array index; every
 *              element of a given array is written): h_residual, the largest
 *              |((p.p - E^2) - f u^2) + 1| / (((E^2 + p.p) + f u^2) + 1) over the start point and
 *              every finite substep end; lz_drift, |L_z,end - L_z,0|; status (int), one of
 *              BHRT_PSTAT_*; substeps (int), the RK4 substeps taken in this call. Particles that did
 *              not run get zeros in h_residual, lz_drift and substeps.
 *  Refusals.   -1 with bhrt_last_error set, nothing written, no state changed and updates
 *              unchanged, each decided BEFORE ANY HIP CALL (the current device's query aside):
 *              everything bhrt_particles_update_device refuses -- a NULL object, blackhole or
 *              config, steps < 0, a current device other than the object's --; |spin| >= 1 or NaN;
 *              mass not finite or not > 0; time_step not finite or not > 0; a NULL params; substeps
 *              outside 1..64. steps == 0 is a no-op that returns 0. HIP failures also return -1.
 *  Streams.    As for bhrt_particles_update_device: asynchronous, NO host wait; NULL is ordered like
 *              the legacy default stream; the caller orders calls on one object.
 *  Not offered. Massless or charged particles; an adaptive (Dormand-Prince) particle step; a host
 *              one-shot on a ParticleSystem (a caller composes create, update and download);
 *              particle-disk interaction; bhrt_stats entries (the parity update has none either). */
#define BHRT_PSTAT_MOVED 0
#define BHRT_PSTAT_CAPTURED 1
#define BHRT_PSTAT_NOT_TIMELIKE 2
#define BHRT_PSTAT_ERROR 3
#define BHRT_PSTAT_INACTIVE 4
typedef struct { int substeps; } bhrt_kerr_particles_params;
typedef struct { double* h_residual; double* lz_drift; int* status; int* substeps; } bhrt_kerr_particles_diag;

int bhrt_particles_kerr_update_device(bhrt_particles* ps, const BlackHoleParams* blackhole,
                                      const SimulationConfig* config, int steps,
                                      const bhrt_kerr_particles_params* params,
                                      const bhrt_kerr_particles_diag* device_diag /* may be NULL */,
                                      void* hip_stream);
/* The velocity-to-momentum paragraph on the host with the device's operations: state = (x, p), *E,
 * *ut. 0; 1 and nothing written if not timelike or r <= r+; -1 for a NULL argument or a bad
 * blackhole as above. No HIP call. */
int bhrt_kerr_particle_state(const BlackHoleParams* blackhole, const Vector3D* position,
                             const Vector3D* velocity, double state[6], double* E, double* ut);
/* Orbit helper: the coordinate velocity of the circular equatorial geodesic through `position` (z
 * must be 0): r = sqrt(x^2 + y^2 - a^2), Omega = +-sqrt(M) / (r sqrt(r) +- a sqrt(M)) (upper sign:
 * prograde, about +z in +phi, the emission rule's Omega), v = Omega (-y, x, 0). 0; 1 and nothing
 * written where no timelike circular orbit exists (r <= r+, or r sqrt(r) - 3 M sqrt(r) +-
 * 2 a sqrt(M) <= 0); -1 for a NULL argument, z != 0 or a bad blackhole. No HIP call. */
int bhrt_kerr_orbit_velocity(const BlackHoleParams* blackhole, const Vector3D* position, int prograde,
                             Vector3D* velocity);

/* Last error message of the calling thread ("" if none). */
const char* bhrt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* BHRT_API_H */
