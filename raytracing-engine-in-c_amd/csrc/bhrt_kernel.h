/*
 * bhrt_kernel.h -- launch parameters shared by the C host layer (bhrt_host.h) and the HIP
 * kernels (geodesic.hip, paths.hip, frames.hip, kerr.hip, particles.hip). Plain C, passed by
 * value as the kernel argument block, so every field is wave-uniform and read through the scalar
 * unit.
 *
 * Everything that is the same for all rays of a launch is computed ONCE on the host with
 * the same IEEE operations the reference performs inline (so identical rounding):
 *   - the scene constants (rs*1.5, dt*0.001, ...);
 *   - for a camera frame, the spherical coordinates of the shared origin (glibc acos /
 *     atan2 / sin / cos, exactly the reference's values) and the metric there.
 */
#ifndef BHRT_KERNEL_H
#define BHRT_KERNEL_H

#include "../../include/bhrt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BHRT_SRC_RAYS = 0, BHRT_SRC_CAMERA = 1 };
enum { BHRT_NUM_COUNTERS = 5 }; /* rays, iterations, stages full/far/kerr */
enum { BHRT_MAX_QUEUE_BITS = 5, BHRT_QUEUE_STRIDE_MAX = 64 }; /* ray queues of k_trace */
enum { BHRT_INIT_FIELDS = 21 }; /* ray arrays: y0..y5, y6, y7, dx, dy, dz, px, py, pz,
                                   far_ok, sin/cos of y1, y2, y3; camera frames use the first
                                   BHRT_INIT_FIELDS_CAMERA rows (the rest is the shared origin) */
enum { BHRT_INIT_FIELDS_CAMERA = 8 }; /* y4, y5, y6, y7, dx, dy, dz, far_ok */
enum { BHRT_SCRATCH_FIELDS = BHRT_INIT_FIELDS + 1 + 3 }; /* a launch's scratch, in doubles per ray:
                                   the init table, the redo list, and the exit chords a sky frame
                                   hands to the separate colour pass (bhrt_sky_k.chord) */

typedef struct {
    /* scene constants (raytracer.c:65-130, 465, 556-571, 652-659; spacetime.c:22) */
    double M, rs, two_m;
    double rs_x1_5, rs_x1_05, rs_x2_5, rs_x5, rs_x15, rs_eps;
    double h_2_5, h_5, h_15, h_far;
    /* the r interval of each step size of the schedule, [h_lo[k], h_hi[k]): k = 0 h_far,
     * 1 h_15, 2 h_5, 3 h_2_5 (an empty interval for a size the select chain never picks) */
    double h_lo[4], h_hi[4];
    double max_dist, tol;
    double disk_in, disk_out, disk_tscale;
    double disk_in_sq, disk_out_sq; /* exact s-bounds of inner <= RN(sqrt(s)) <= outer */
    int max_steps;
    int method;  /* IntegrationMethod */
    int has_disk;
    int flags;   /* BHRT_FLAG_* */
    int spin0;   /* blackhole->spin == 0.0 */
    int far_bounded; /* a state within 2^40 stays below 2^400 over max_steps steps, far-field
                        branch included (scene.c far_bounded; bhrt_trace_core.h
                        repair_at_refill) */
    double rot_vmax; /* zero-acceleration paths: a ray with |state[5]| below this turns state[2]
                        by less than pi/4 per step for every step size (bhrt_trace_core.h
                        rotation_trig); a ray at or above it is re-traced by the redo pass */
    int accept_all;  /* RKF45 with 2^-30 <= tol <= 2^300 and finite step sizes: no attempt on the
                        zero-acceleration paths can be rejected (bhrt_trace_core.h rkf45_attempt
                        ACC) */
    double m_4;      /* M / 4: the a = 0 stage forms -M / r^2 from -2 / r (bhrt_trace_core.h
                        rhs) */
} bhrt_scene_k;

typedef struct {
    /* pixel -> direction (calculate_ray_direction, raytracer.c:999-1039) */
    double fwd[3], right[3], up[3];
    double plane_w, plane_h;
    double off_x, off_y;             /* sub-pixel offset (0.5, 0.5 = centre)   */
    int width, height;
    bhrt_rows rows;
    double inv_width, inv_block;     /* RN(1 / width), RN(1 / rows.row_block)  */
    /* shared origin (integrate_photon_path set-up, raytracer.c:355-466); also filled for ray
     * arrays with one origin (bhrt_kparams.rays_shared) */
    double pos[3];                   /* Cartesian origin                        */
    double r0, th0, ph0;             /* cartesian_to_spherical(origin)          */
    double st_cp, st_sp, ct, ct_cp, ct_sp, st, neg_sp, cp, r_st; /* trig products */
    double g_tt, g_rr, g_hh;         /* calculate_schwarzschild_metric(r0)      */
    double p0[3];                    /* spherical_to_cartesian(r0, th0, ph0)    */
    double sp;                       /* sin(ph0)                                */
    double s_r0, c_r0;               /* sin, cos(r0): state[1] as ray_derivatives' theta */
    int use_approx;                  /* r0 > 15 rs                              */
    int st_tiny;                     /* fabs(sin th0) < BH_EPSILON              */
    /* claim order: the shard's pixels in tiles of 2^tile_w_log2 x 2^tile_h_log2 = 64 pixels
     * (one wavefront), tiles row-major; tiles_per_row == 0: ray id order */
    int tile_w_log2, tile_h_log2, tiles_per_row;
    double inv_tiles_per_row;        /* RN(1 / tiles_per_row)                   */
    int ntiles, tile_stride;         /* tile_stride > 0: the claim order visits tile
                                        (t * tile_stride) mod ntiles at step t (scatter) */
} bhrt_camera_k;

/* The bound sky map of a launch with BHRT_FLAG_SKY (the rule: include/bhrt_api.h "Sky maps"); all
 * zero otherwise. The record is the calling thread's (scene.c bhrt_sky_bind), copied here by
 * bhrt_fill_scene; the kernels read it at a ray's exit only (bhrt_colour.h sky_lookup). */
typedef struct {
    const void* tex;      /* device [h][w] texels, 16 bytes each: r, g, b as float and a pad, so
                             one tap is one aligned load; NULL: no sky */
    int w, h;
    double sx, sy;        /* RN(w / (2 pi)), RN(h / pi): texels per radian */
    double* chord;        /* the separate colour pass only (colour_fused == 0): [3][n] scratch,
                             the exit chord of every RAY_MAX_DISTANCE ray (set per launch) */
} bhrt_sky_k;

/* Whether the trace kernel writes a scene's colour outputs at each ray's exit, from the state in
 * registers (no separate colour pass re-reading the hits). Every scene does: the separate pass
 * of a frame could only start once the trace kernel's last wave had ended, by when the next
 * frame's persistent workgroups held every wave slot, so a C2 frame's colour landed ~1 frame
 * late (k_colour dispatches averaged 5.5 ms), and fusing costs nothing (C2 284.5 vs 284.6
 * Mrays/s same box, profiles/r06/ab_fused_colour.txt; C5 +16%, C1 +9%). Scenes without a disk
 * get the sky / horizon colour alone (bhrt_colour.h colour_sky). BHRT_FUSE_COLOUR=0 at run time
 * takes the separate pass (A/B, and the tests' reference path). */

typedef struct {
    bhrt_scene_k sc;
    int src;              /* BHRT_SRC_*                                       */
    int n;                /* rays in this launch                              */
    int refill;           /* refill a wave once >= refill lanes are idle      */
    int claim_min;        /* smallest block of ray ids a wave claims at once (multiple of 64) */
    int claim_div;        /* a claim takes (unclaimed rays) / (waves * claim_div), at least
                             claim_min: large blocks while the queue is full, small at the end */
    const Ray* rays;      /* BHRT_SRC_RAYS: device AoS input                  */
    double* init;         /* [BHRT_INIT_FIELDS][n] initial state (k_init)      */
    int* redo;            /* [n] ids of rays re-traced with the large-argument path */
    bhrt_camera_k cam;    /* BHRT_SRC_CAMERA                                  */
    bhrt_frame_soa out;   /* device SoA outputs; NULL fields skipped          */
    unsigned long long* ctl; /* [1..5] counters, [6] redo count, [7] redo queue head; the
                                launch's slot of the control ring, zero at launch (the ring is
                                filled with zeros on the GPU after each harvest, context.c
                                ring_order) */
    unsigned long long* qhead; /* ray-queue heads, queue q at qhead[q * queue_stride]; same slot */
    int queue_bits;       /* 2^queue_bits ray queues (<= BHRT_MAX_QUEUE_BITS)            */
    int queue_stride;     /* u64 words between queue heads (<= BHRT_QUEUE_STRIDE_MAX)     */
    int claim_shift;      /* set by the launcher per launch: a block claim is the queue's
                             remainder >> claim_shift, 2^claim_shift >= waves * claim_div / queues */
    int colour_fused;     /* the trace kernel writes the colour outputs (rgb, rgba32f, rgba8)
                             of each ray at its exit; else a separate colour pass runs */
    const int* order;     /* camera frames: the claim order, queue position -> ray id (a
                             permutation of [0, n)); NULL = ray id order */
    int skip_redo;        /* the redo launch may be left out where no ray can be evicted
                             (geodesic.hip launch_trace_pair); BHRT_SKIP_REDO=0: always launch */
    int no_evict;         /* the host proved that no ray of this launch can be handed to the
                             redo pass (scene.c origin_no_evict; camera frames and ray
                             arrays with one shared origin) */
    int block_lanes;      /* lanes per workgroup of the hot trace launch (64, 128 or 256) */
    int rays_shared;      /* BHRT_SRC_RAYS whose every origin is cam.pos (the host checked):
                             cam's origin block is filled as for a camera frame, and the
                             trace kernel sets rays up from their directions (no k_init) */
    const double* dirs;   /* rays_shared: ray i's direction at dirs[i * dir_stride + 0..2]
                             (the AoS rays' direction field, stride 6, or packed, stride 3,
                             with rays NULL) */
    int dir_stride;
    int grid_div;         /* > 0: the hot launch takes 1 / grid_div of the resident workgroups */
    int grid_blocks;      /* > 0: at most this many workgroups in the hot launch (A/B knob) */
    int min_tiles;        /* drained-refill launches of fewer 64-ray tiles per resident wave
                             than this take half the grid (0 = off) */
    int diag_slot;        /* the launch's control-block slot (the BHRT_WAVE_STAMPS diagnostic
                             build records per-wave stamps under it; unused otherwise) */
    bhrt_sky_k sky;       /* sc.flags & BHRT_FLAG_SKY: the sky map. Last, so that every other
                             field keeps its place in the kernel argument segment */
} bhrt_kparams;

/* Supersampled camera frames (supersample.c; frames.hip k_ss_rays, k_ss_resolve): two
 * elementwise kernels around ONE shared-origin trace of n * samples rays. The sample rays are
 * sample-major -- ray s * n + p is shard pixel p (camera_dir's index) at sample s -- so sample
 * plane s is exactly the frame at offset s. k_ss_rays is launched once per sample, the sample's
 * offset by value in the argument block's camera, and reads that camera in place as k_trace and
 * k_colour read theirs: with the offset patched into a local copy of the block hipcc contracted
 * camera_dir's squared length in another order (x*x first instead of y*y), one ulp off the
 * camera path's directions. */
typedef struct {
    bhrt_camera_k cam;    /* basis, image plane and row shard (fill_camera); off_x/off_y: the
                             sample's sub-pixel offset */
    int n, sample;        /* shard pixels; the sample s: this launch writes rays [s n, s n + n) */
    double* dirs;         /* [n * samples][3] packed directions (the trace's kp.dirs) */
} bhrt_ss_rays_k;

typedef struct {
    int n, samples;
    const int32_t* result;      /* [samples][n] sample planes written by the trace */
    const double *r, *g, *b;
    bhrt_frame_soa out;         /* result, rgb_r/g/b, rgba32f, rgba8; NULL fields skipped */
} bhrt_ss_resolve_k;

/* frames.hip; asynchronous on `stream`; return 0 or a hipError_t value */
int bhrt_launch_ss_rays(const bhrt_ss_rays_k* k, void* stream);
int bhrt_launch_ss_resolve(const bhrt_ss_resolve_k* k, void* stream);

/* Adaptive supersampled frames (adaptive.c; frames.hip k_ad_rays, k_ad_edges, k_ad_resolve;
 * the rule is stated in bhrt_api.h). Rays are addressed by IMAGE pixel: the camera block is the
 * whole image's (rows = {0, 0, 1}), and the shard enters through two row tables.
 *   ext rows   the image rows the base pass traces, ascending: the shard's own rows and its
 *              halo rows; ext pixel q = e * width + px. rows[e] is ext row e's image row and
 *              ext_of[y] image row y's ext row (or -1); both NULL for a whole image (identity).
 *   base planes  [B][next] sample-major over the ext pixels, written by the first trace.
 *   extra planes [M - B][E] over the edge list's slots, written by the second. */
typedef struct {
    bhrt_camera_k cam;    /* the whole image's camera; off_x/off_y: the sample's offset, read in
                             place as k_ss_rays reads its own */
    int n;                /* rays of this launch                                             */
    long first;           /* ray r's direction goes to dirs[(first + r) * 3 ..]               */
    const int* rows;      /* base pass: ray r is ext pixel r (NULL: image pixel r)            */
    const int* pixels;    /* extra pass: ray r is image pixel pixels[r] (the edge list)       */
    double* dirs;
} bhrt_ad_rays_k;

typedef struct {
    int n, width, height; /* owned pixels; the image                                         */
    bhrt_rows rows;       /* the shard (num_shards <= 1: whole image)                        */
    double inv_width, inv_block;
    const int* ext_of;    /* [height] or NULL                                                */
    long next;            /* ext pixels: the base planes' stride                             */
    int base, max;        /* B, M                                                            */
    double threshold;
    const double *r, *g, *b; /* base planes                                                  */
    int* slot;            /* [n] out: the pixel's slot in the edge list, or -1                */
    int* list;            /* [n] out: slot -> image pixel                                    */
    unsigned long long* count; /* edge pixels so far (zero at launch)                        */
} bhrt_ad_edges_k;

typedef struct {
    int n, width, height;
    bhrt_rows rows;
    double inv_width, inv_block;
    const int* ext_of;
    long next, nedge;     /* ext pixels; E, the extra planes' stride                          */
    int base, max;
    const int32_t* result;   /* base class planes (plane 0 is the pixel's class)               */
    const double *r, *g, *b; /* base planes                                                  */
    const double *xr, *xg, *xb; /* extra planes (unused where nedge == 0 or max == base)       */
    const int* slot;
    bhrt_frame_soa out;   /* result, rgb_r/g/b, rgba32f, rgba8; NULL fields skipped           */
    int32_t* samples;     /* S(p), or NULL                                                   */
} bhrt_ad_resolve_k;

/* frames.hip; asynchronous on `stream`; return 0 or a hipError_t value */
int bhrt_launch_ad_rays(const bhrt_ad_rays_k* k, void* stream);
int bhrt_launch_ad_edges(const bhrt_ad_edges_k* k, void* stream);
int bhrt_launch_ad_resolve(const bhrt_ad_resolve_k* k, void* stream);

/* Temporal accumulation (temporal.c; frames.hip k_ta_blend, k_ta_edges; the rule is stated in
 * bhrt_api.h). Two elementwise kernels behind the unchanged camera-frame launch: the blend with
 * the display conversion, then -- whole images only -- the edge stencil on the UPDATED acc, a
 * launch of its own because the blend updates acc in place (a lane that recomputed its
 * neighbours' blends would race with their stores unless acc were kept twice). */
typedef struct {
    long n;               /* pixels                                                          */
    const float* frame;   /* the new frame: [n][4] (the trace's rgba32f) or [n][3]            */
    int stride;           /* 4 or 3                                                          */
    int zero;             /* step 1: acc counts as 0.0f, whatever the array holds             */
    float alpha, w;       /* step 2's alpha and w = 1.0f - alpha, rounded on the host          */
    float* acc;           /* [n][3] in place                                                 */
    float* rgb;           /* [n][3] copy of the new acc, or NULL                              */
    uint8_t* rgba8;       /* [n][4] step 6, or NULL                                           */
} bhrt_ta_blend_k;

typedef struct {
    long n;               /* width * height                                                  */
    int width, height;
    float threshold, decay;
    const float* acc;     /* [n][3] the updated acc                                          */
    float* edge;          /* [n] in place (border pixels are never written: they stay 0)       */
    float* out;           /* [n] copy of the new edge, or NULL                                */
} bhrt_ta_edges_k;

/* frames.hip; asynchronous on `stream`; return 0 or a hipError_t value */
int bhrt_launch_ta_blend(const bhrt_ta_blend_k* k, void* stream);
int bhrt_launch_ta_edges(const bhrt_ta_edges_k* k, void* stream);

/* Batched photon paths (paths.c; paths.hip k_paths): the launch's bhrt_kparams carries the
 * scene, the AoS rays, n and the control block (ctl[0]: the claim counter, ctl[1..5]: the
 * statistics, as k_trace's; its hit outputs are not used); this block the path outputs. */
#ifndef BHRT_PATHS_STAGED /* the default store form: 1 staged through LDS, 0 direct (the faster
                             on both measured batches: C4 0.155 vs 0.186 ms per 4096 rays,
                             profiles/paths/bench_paths.jsonl); BHRT_PATHS_STORE picks at run time */
#define BHRT_PATHS_STAGED 0
#endif
enum { BHRT_PATHS_RING = 8 }; /* staged form: points a lane holds in LDS between flushes */
typedef struct {
    int max_positions, every;
    int staged;           /* store form of this launch (both are always built) */
    bhrt_paths out;       /* device arrays; NULL fields skipped */
} bhrt_paths_k;

/* paths.hip; asynchronous on `stream`, ev0/ev1 (hipEvent_t, may be NULL) recorded around the
 * kernel; returns 0 or a hipError_t value */
int bhrt_launch_paths(const bhrt_kparams* kp, const bhrt_paths_k* pk, void* stream, void* ev0,
                      void* ev1);

/* update_particles (particle_sim.c:505-566) constants, from the BlackHoleParams and
 * SimulationConfig of the call */
typedef struct {
    double M, rs, a, r_plus; /* mass, schwarzschild_radius, spin * mass, r_plus */
    double dt;               /* config->time_step                                 */
    int spin0;               /* blackhole->spin == 0.0                            */
} bhrt_particle_k;

/* particles.hip: `steps` updates of d_particles[0, count) on `stream`, ev0/ev1 (hipEvent_t,
 * may be NULL) recorded around the kernel; returns 0 or a hipError_t value. */
int bhrt_launch_particles(Particle* d_particles, int count, const bhrt_particle_k* k, int steps,
                          void* stream, void* ev0, void* ev1);

/* Device-resident particle systems (particles_resident.c; the rule: include/bhrt_api.h). All
 * asynchronous on `stream`, ev0/ev1 as above, 0 or a hipError_t value. With nblocks =
 * (count + 255) / 256, the 256-lane workgroups of the update:
 *   _counted  bhrt_launch_particles' update, and d_block_active[b] = workgroup b's particles active
 *             after it (d_block_active [nblocks]);
 *   _count    d_block_active of the array as it stands, no update;
 *   _scan     d_offsets [nblocks + 1] = the exclusive scan of d_block_active, the total last; one
 *             workgroup, no workgroup waits for another;
 *   _scatter  bh_get_particle_data into the DEVICE arrays of `out` by those offsets. */
int bhrt_launch_particles_counted(Particle* d_particles, int count, const bhrt_particle_k* k,
                                  int steps, int* d_block_active, void* stream, void* ev0,
                                  void* ev1);
int bhrt_launch_particles_count(const Particle* d_particles, int count, int* d_block_active,
                                void* stream);
int bhrt_launch_particles_scan(const int* d_block_active, int nblocks, int* d_offsets, void* stream,
                               void* ev0, void* ev1);
int bhrt_launch_particles_scatter(const Particle* d_particles, int count, const int* d_offsets,
                                  int max_count, const bhrt_particle_data* out, void* stream,
                                  void* ev0, void* ev1);

/* Sky lookups by themselves (sky.c; frames.hip k_sky_lookup): rgb[i] = the lookup of dirs[i],
 * n > 0 directions, asynchronous on `stream`; 0 or a hipError_t value */
int bhrt_launch_sky(const bhrt_sky_k* sky, const double* d_dirs, int n, double* d_rgb,
                    void* stream);

/* Physical geodesics (kerr.c; kerr.hip k_kerr; the rule: include/bhrt_api.h "Physical
 * geodesics"). The launch's bhrt_kparams carries the source (src, n, rays or cam -- basis, image
 * plane, row shard and cam.pos, the shared origin), the outputs, the control block (ctl[0]: the
 * claim counter, ctl[1..2]: rays and RK4 steps, ctl[8..9]: the execution window) and what the
 * colour reads (sc.flags, sc.rs, sc.has_disk, sc.disk_in / disk_out / disk_tscale, sky); this
 * block the integration's constants, each formed once on the host. */
typedef struct {
    double M, two_m;      /* mass, 2 M                                                      */
    double a, a2;         /* a~ = -(spin * mass), a~^2                                       */
    double r_plus;        /* M + sqrt(M^2 - a~^2)                                            */
    double eight_m;       /* 8 M: the step size reads r / (8 M)                             */
    double dt, max_dist;  /* time_step, max_ray_distance                                    */
    double disk_lo, disk_hi; /* in^2 + a~^2, out^2 + a~^2: the bounds of q_x^2 + q_y^2      */
    int max_steps, has_disk;
    int tiles_x, ntiles;  /* camera frames: 8x8 tiles per row of tiles, tiles in the shard   */
    int nrows;            /* camera frames: the shard's rows                                 */
    double* h_residual;   /* bhrt_kerr_diag, device [n] or NULL                              */
    double* lz_drift;
} bhrt_kerr_k;

/* kerr.hip; asynchronous on `stream`, ev0/ev1 (hipEvent_t, may be NULL) recorded around the
 * kernel; returns 0 or a hipError_t value */
int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream, void* ev0,
                     void* ev1);

/* Physical photon paths (kerr_paths.c; kerr.hip k_kerr_paths; the rule: include/bhrt_api.h
 * "Physical photon paths"). The launch's bhrt_kparams carries the AoS rays, n and the control block
 * (ctl[0]: the claim counter, ctl[1..2]: rays and RK4 steps, ctl[8..9]: the execution window; its
 * outputs, scene and sky map are not read); this block the integration's constants -- the ones
 * bhrt_launch_kerr gets for the same scene -- and the path outputs. */
typedef struct {
    bhrt_kerr_k k;        /* tiles, rows and the diag pointers are not read */
    int max_positions, every;
    bhrt_paths out;       /* device arrays; NULL fields skipped */
} bhrt_kerr_paths_k;

/* kerr.hip; as bhrt_launch_kerr */
int bhrt_launch_kerr_paths(const bhrt_kparams* kp, const bhrt_kerr_paths_k* pk, void* stream,
                           void* ev0, void* ev1);

/* Physical geodesics, adaptive steps (kerr_rk45.c; kerr.hip k_kerr_rk45; the rule:
 * include/bhrt_api.h "Physical geodesics, adaptive steps"). bhrt_kparams as for bhrt_launch_kerr
 * (ctl[2] counts attempts); this block the constants bhrt_launch_kerr gets for the same scene
 * (k.dt: the first trial step; k.eight_m is not read), the tolerance and the extra plane. */
typedef struct {
    bhrt_kerr_k k;
    double tol;           /* config->tolerance, checked: finite, in [1e-12, 1e-2]            */
    int* rejected;        /* bhrt_kerr_rk45_diag.rejected, device [n] or NULL                */
} bhrt_kerr_rk45_k;

/* kerr.hip; as bhrt_launch_kerr */
int bhrt_launch_kerr_rk45(const bhrt_kparams* kp, const bhrt_kerr_rk45_k* rk, void* stream,
                          void* ev0, void* ev1);

/* Kerr disk emission (kerr_emit.c; kerr.hip k_kerr_emit; the rule: include/bhrt_api.h "Kerr disk
 * emission"). bhrt_kparams as for bhrt_launch_kerr_rk45 (sc.flags never has BHRT_FLAG_DOPPLER;
 * sc.disk_in is the emissivity's reference radius); this block the adaptive launch's, the
 * emission's parameters and its outputs. */
typedef struct {
    bhrt_kerr_rk45_k rk;
    int max_crossings;    /* K, checked: 1..BHRT_EMIT_MAX_CROSSINGS                          */
    double q, gain;       /* emissivity_index, gain; checked: finite, >= 0                   */
    double spin_a;        /* spin * mass, the physical spin (-rk.k.a)                        */
    bhrt_kerr_emit_out out; /* device arrays; NULL fields skipped; radius, redshift [K][n]   */
} bhrt_kerr_emit_k;

/* kerr.hip; as bhrt_launch_kerr */
int bhrt_launch_kerr_emit(const bhrt_kparams* kp, const bhrt_kerr_emit_k* ek, void* stream,
                          void* ev0, void* ev1);

/* Physical particles (kerr_particles.c; kerr.hip k_kerr_particles; the rule: include/bhrt_api.h
 * "Physical particles"). k holds the constants bhrt_launch_kerr gets for the same scene with
 * a = +(spin * mass) -- particles run forward in time --; of it M, two_m, a, a2, r_plus, eight_m
 * and dt are read, and h_residual / lz_drift are bhrt_kerr_particles_diag's planes. */
typedef struct {
    bhrt_kerr_k k;
    int substeps;         /* params->substeps, checked: 1..64                                 */
    int* status;          /* bhrt_kerr_particles_diag.status, device [count] or NULL          */
    int* substeps_out;    /* bhrt_kerr_particles_diag.substeps, device [count] or NULL        */
} bhrt_kerr_particles_k;

/* kerr.hip: `steps` ticks of d_particles[0, count) in 256-lane workgroups, and d_block_active[b] =
 * workgroup b's particles active after them, as bhrt_launch_particles_counted leaves it;
 * asynchronous on `stream`, ev0/ev1 (hipEvent_t, may be NULL) recorded around the kernel; 0 or a
 * hipError_t value */
int bhrt_launch_kerr_particles(Particle* d, int count, const bhrt_kerr_particles_k* k, int steps,
                               int* d_block_active, void* stream, void* ev0, void* ev1);

/* launch helpers implemented in geodesic.hip; return 0 or a hipError_t value.
 * bhrt_launch_trace records ev0/ev1 (hipEvent_t, may be NULL) around the trace kernel
 * itself, not the set-up or colour passes. */
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1);
/* 1 if bhrt_launch_trace runs kp's RKF45 attempts without the accept test (bhrt_stats) */
int bhrt_trace_untested(const bhrt_kparams* kp);
/* paths.hip (k_path); return 0 or a hipError_t value */
int bhrt_launch_path(const bhrt_kparams* kp, const double* origin4, const double* dir3,
                     Vector3D* d_path, int max_positions, int* d_num, int num_positions_in,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
