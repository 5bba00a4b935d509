/*
 * scene.c -- a launch's scene, camera and origin set-up (bhrt_kparams): the products the
 * reference forms inline, the claim policy, and the proofs that let the kernels leave work out
 * (far_bounded, origin_no_evict, the square-root-free disk bounds). Pure host arithmetic with the
 * reference's libm calls; nothing outside this file is allowed to affect a frame's bits.
 */
#include <math.h>
#include <string.h>

#include "bhrt_host.h"

static int g_refill = 0; /* 0: chosen per scene (refill_default) */

void bhrt_set_refill_threshold(int lanes) {
    g_refill = lanes <= 0 ? 0 : (lanes > 64 ? 64 : lanes);
}

/* Refill threshold by the expected ray lifetime. RK4 on a = 0: lifetimes
 * spread over 1..max_steps iterations (C2), so idle lanes are refilled early (8). Otherwise
 * (Kerr: straight-line stages; RKF45: fixed point after a few attempts) rays are short-lived
 * and similar, each refill is an HBM-latency stall, and a wave refills only once drained. */
static int refill_default(const bhrt_scene_k* s) {
    const int r = bhrt_env_int("BHRT_REFILL", 0); /* A/B override */
    if (r >= 1 && r <= 64) return r;
    return (s->method == INTEGRATOR_RK4 && s->spin0) ? 8 : 64;
}

/* The trace kernel writes the colour outputs at each ray's exit, from the state in registers
 * (bhrt_kernel.h), so the separate pass's inputs -- result and hit point -- need not exist on
 * the device. BHRT_FUSE_COLOUR=0 keeps the separate colour pass (A/B), for every scene alike. */
int bhrt_colour_fused(int method, int has_disk, int spin) {
    return bhrt_env_int("BHRT_FUSE_COLOUR", 1) != 0;
}

/* Ray queues of k_trace: 2^queue_bits queue heads, queue_stride words apart,
 * and the claim policy. Every claim is a returning device-scope atomic, and claims on ONE word
 * serialise at the memory side (~65 M/s): with one queue, C3 (2 M rays of ~2 iterations) ran
 * at exactly that claim rate. 16 queues: C3 +75%. Where a wave refills only once drained
 * (refill 64: short-lived rays), a claim also takes a block of ids for the next refills
 * (claim_div 1: C3 another +25%, C4 +2%); where lanes are refilled as they finish (C2: rays
 * of 1..1000 iterations) a claim takes exactly the idle lanes -- a block claimed from a stale
 * estimate of the remainder would hold long rays back into the frame's tail (C2 -17%).
 * Same-box sweep: profiles/r02_claim_sweep.txt. BHRT_QUEUES (a power of two),
 * BHRT_QUEUE_STRIDE (words), BHRT_CLAIM_MIN / BHRT_CLAIM_DIV (0 = exactly the idle lanes)
 * override the defaults. */
static void claim_policy(bhrt_kparams* kp) {
    int q = bhrt_env_int("BHRT_QUEUES", 16), bits = 0;
    while (bits < BHRT_MAX_QUEUE_BITS && (2 << bits) <= q) bits++;
    int stride = bhrt_env_int("BHRT_QUEUE_STRIDE", 32);
    if (stride < 1) stride = 1;
    if (stride > BHRT_QUEUE_STRIDE_MAX) stride = BHRT_QUEUE_STRIDE_MAX;
    int m = bhrt_env_int("BHRT_CLAIM_MIN", 64), d = bhrt_env_int("BHRT_CLAIM_DIV", kp->refill >= 64);
    if (m < 64) m = 64;
    if (m > 1 << 16) m = 1 << 16;
    kp->queue_bits = bits;
    kp->queue_stride = stride;
    kp->claim_min = (m + 63) & ~63;
    kp->claim_div = d < 0 ? 0 : d;
}

int bhrt_check_scene(const BlackHoleParams* bh, const SimulationConfig* cfg) {
    if (!bh || !cfg) {
        set_err("blackhole and config must not be NULL");
        return -1;
    }
    return 0;
}

/* the colour pass (rgb and/or the display fields) reads result and the hit point */
int bhrt_colour_args_bad(const bhrt_frame_soa* out, int method, int has_disk, int spin) {
    if ((out->rgb_r || out->rgb_g || out->rgb_b) && !(out->rgb_r && out->rgb_g && out->rgb_b)) {
        set_err("rgb output needs all of rgb_r/g/b");
        return 1;
    }
    if ((out->rgb_r || out->rgba32f || out->rgba8) && !bhrt_colour_fused(method, has_disk, spin) &&
        (!out->result || !out->hit_x || !out->hit_y)) {
        set_err("colour outputs need result and hit_x/hit_y (separate colour pass)");
        return 1;
    }
    return 0;
}

/* The disk test's inner <= sqrt(qx^2+qy^2) <= outer (raytracer.c:190-191) without the square
 * root: sqrt is correctly rounded and monotone, so {s : RN(sqrt(s)) >= inner} = {s >= lo} and
 * {s : RN(sqrt(s)) <= outer} = {s <= hi} for the thresholds found here by stepping from the
 * rounded square (a few ulps). NaN bounds keep the comparisons false, as in the reference. */
static double sqrt_lower_bound(double inner) {
    if (isnan(inner)) return NAN;
    if (inner <= 0.0) return -INFINITY;
    double s = inner * inner;
    while (s > 0.0 && sqrt(nextafter(s, 0.0)) >= inner) s = nextafter(s, 0.0);
    while (sqrt(s) < inner) s = nextafter(s, INFINITY);
    return s;
}

static double sqrt_upper_bound(double outer) {
    if (isnan(outer)) return NAN;
    if (outer < 0.0) return -INFINITY;
    if (isinf(outer)) return INFINITY;
    double s = outer * outer;
    while (sqrt(s) > outer) s = nextafter(s, 0.0);
    while (!isinf(s) && sqrt(nextafter(s, INFINITY)) <= outer) s = nextafter(s, INFINITY);
    return s;
}

/* Whether every state the trace loop can reach from an initial state within 2^40 stays below
 * 2^400 for max_steps steps with the far-field branch taking part (bhrt_trace_core.h
 * repair_at_refill: the far-field instantiations then run the state recovery once per ray and
 * the division-free RKF45 accept test). Stage accelerations are clamped to 10, zero, or -- in
 * the far-field branch, only where y0 > 15 rs -- y5 * 2M / y0^2 with a factor below
 * C = 2M / (15 rs)^2. With h the largest step size, S = 18 >= the largest stage weight sum of
 * RK4 (1) and RKF45 (17.4), W = 1.5 >= the final combination's (RK4 1, RKF45 1.4) and q = h S C
 * < 1/2, a stage velocity is at most 2 (V + 10 h S) for velocities V at the step's start, so
 * V' <= g V + a with g = 1 + 2 h W C, a = 20 h W: V_N <= g^N (V_0 + N a); the position moves
 * by at most 2 h W (V + 10 h S) per step. */
static int far_bounded(const bhrt_scene_k* s) {
    if (s->max_steps <= 0) return 1;
    if (!(s->two_m >= 0.0) || !(s->rs_x15 > 0.0 || s->two_m == 0.0)) return 0;
    const double C = s->two_m == 0.0 ? 0.0 : s->two_m / (s->rs_x15 * s->rs_x15) * (1.0 + 1e-9);
    const double h = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
    const double S = 18.0, W = 1.5, N = (double)s->max_steps;
    if (!isfinite(C) || !isfinite(h) || !(h * S * C < 0.5)) return 0;
    const double logv = log2(0x1p40 + N * 20.0 * h * W) + N * log1p(2.0 * h * W * C) / log(2.0);
    const double logp = log2(0x1p40 + N * 2.0 * h * W * (exp2(fmin(logv, 1000.0)) + 10.0 * h * S));
    return logv <= 400.0 && logp <= 400.0;
}

/* Whether no ray that starts at this origin can be handed to the redo pass (geodesic.hip k_trace:
 * a finite sincos argument |x| >= 2^20, a far-field state the host could not prove bounded, or
 * -- on the zero-acceleration Kerr paths -- |state[5]| >= rot_vmax). Then the redo launch is
 * left out (launch_trace_pair): one dispatch less per frame, and a frame's completion no longer
 * waits behind the next frame's persistent workgroups for a wave slot.
 * The live state is (t, r, theta, phi, tdot, rdot); ray_derivatives reads it shifted, so the
 * derivatives of components 0..2 are components 3..5 ("velocities" V) and those of 3..5 are
 * accelerations: clamped to 10, zero (Kerr), or -- far-field branch, only where y0 > 15 rs --
 * y5 * 2M / y0^2 with a factor below C = 2M / (15 rs)^2. With h the largest step size, S the
 * largest stage weight sum (RK4 1, RKF45 17.4 -> 18) and W the final combination's (RK4 1,
 * RKF45 1.4 -> 1.5): without the far-field branch a stage velocity is at most V + 10 h S, a step
 * moves V by at most 10 h W and the positions P by at most h W (V + 10 h S); with it (q = h S C
 * < 1/2) a stage velocity is at most 2 (V + 10 h S), V' <= g V + 20 h W with g = 1 + 2 h W C,
 * and P moves by at most 2 h W (V + 10 h S) (far_bounded's argument). The initial state: t = 0,
 * r, theta, phi of the origin, rdot = n.e_r <= 1 and tdot^2 <= (|g_rr| + (g_hh / r^2)(1 + 1 /
 * sin^2 theta)) / |g_tt| (n a unit vector; its components on the orthonormal e_theta, e_phi
 * give theta-dot = n.e_theta / r, phi-dot = n.e_phi / (r sin theta)). Every sincos argument
 * of the loop is a (stage) value of components 1..3, so a bound below 2^20 proves the claim. */
static int origin_no_evict(const bhrt_scene_k* s, double r, double th, double ph, double st,
                           int st_tiny, double g_tt, double g_rr, double g_hh, int far) {
    if (s->max_steps <= 0) return 1;
    const int rkf = s->method == INTEGRATOR_RKF45;
    if (!rkf && s->method != INTEGRATOR_RK4) return 1; /* (no-op integrators: no step at all) */
    if (!s->spin0 && !far) /* the rotation paths: no sincos in the loop; |rdot| <= 1 + 2^-50 */
        return s->rot_vmax > 1.001;
    if (far && !s->far_bounded) return 0;
    if (!(isfinite(r) && isfinite(th) && isfinite(ph) && isfinite(g_tt) && isfinite(g_rr) &&
          isfinite(g_hh) && g_tt != 0.0 && r != 0.0))
        return 0;
    const double h = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
    if (!isfinite(h)) return 0;
    const double S = rkf ? 18.0 : 1.0, W = rkf ? 1.5 : 1.0, N = (double)s->max_steps;
    const double sl = 1.0 + 1e-6; /* slack for the rounding of the set-up's products */
    const double inv_st2 = st_tiny ? 0.0 : 1.0 / (st * st);
    if (!isfinite(inv_st2)) return 0;
    const double vt2 = (fabs(g_rr) + fabs(g_hh) / (r * r) * (1.0 + inv_st2)) / fabs(g_tt);
    const double V0 = fmax(fmax(fabs(ph), sqrt(vt2) * sl), sl);
    const double P0 = fmax(fabs(r), fabs(th));
    double V, P, B;
    if (!far || s->two_m == 0.0) {
        V = V0 + N * 10.0 * h * W;
        P = P0 + N * h * W * (V + 10.0 * h * S);
        B = fmax(P + h * S * (V + 10.0 * h * S), V + 10.0 * h * S);
    } else {
        const double C = s->two_m / (s->rs_x15 * s->rs_x15) * (1.0 + 1e-9);
        if (!isfinite(C) || !(h * S * C < 0.5)) return 0;
        const double lg = N * log1p(2.0 * h * W * C);
        if (!(lg < 40.0)) return 0;
        V = exp(lg) * (V0 + N * 20.0 * h * W);
        P = P0 + N * 2.0 * h * W * (V + 10.0 * h * S);
        B = fmax(P + 2.0 * h * S * (V + 10.0 * h * S), 2.0 * (V + 10.0 * h * S));
    }
    return isfinite(B) && B * sl < 1048576.0;
}

/* The calling thread's bound sky map (bhrt_set_sky, sky.c): the record a launch with
 * BHRT_FLAG_SKY copies into its parameters, and the device that holds the texels. Kept here, in
 * the host core, so that no core file names a sky launcher. */
static __thread bhrt_sky_k g_sky;
static __thread int g_sky_dev = -1;

void bhrt_sky_bind(const bhrt_sky_k* k, int device) {
    if (k) g_sky = *k;
    else memset(&g_sky, 0, sizeof g_sky);
    g_sky_dev = k ? device : -1;
}

const void* bhrt_sky_bound(void) { return g_sky.tex; }

int bhrt_sky_check(int flags, int device) {
    if (!(flags & BHRT_FLAG_SKY)) return 0;
    if (!g_sky.tex) {
        set_err("BHRT_FLAG_SKY: no sky map is bound on this thread (bhrt_set_sky)");
        return -1;
    }
    if (device != g_sky_dev) {
        set_err("BHRT_FLAG_SKY: the bound sky map lives on device %d, the launch is for device %d",
                g_sky_dev, device);
        return -1;
    }
    return 0;
}

int bhrt_fill_scene(bhrt_kparams* kp, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, IntegrationMethod method, int flags) {
    memset(kp, 0, sizeof *kp);
    if (flags & BHRT_FLAG_SKY) { /* before any launch of the call: the launch's device is current */
        if (bhrt_sky_check(flags, bhrt_current_device())) return -1;
        kp->sky = g_sky;
    }
    bhrt_scene_k* s = &kp->sc;
    const double rs = bh->schwarzschild_radius, dt = cfg->time_step;
    /* the products the reference forms inline (raytracer.c:65-130, 465, 556-571, 652) */
    s->M = bh->mass;
    s->rs = rs;
    s->two_m = 2.0 * bh->mass;
    s->m_4 = 0.25 * bh->mass; /* exact for every mass of 2^-1020 and above */
    s->rs_x1_5 = rs * 1.5;
    s->rs_x1_05 = rs * 1.05;
    s->rs_x2_5 = rs * 2.5;
    s->rs_x5 = rs * 5.0;
    s->rs_x15 = rs * 15.0;
    s->rs_eps = rs + BH_EPSILON;
    /* the schedule's candidates with fmin(h, 0.1) applied (raytracer.c:556-571) */
    s->h_2_5 = fmin(dt * 0.001, 0.1);
    s->h_5 = fmin(dt * 0.01, 0.1);
    s->h_15 = fmin(dt * 0.1, 0.1);
    s->h_far = fmin(dt, 0.1);
    /* the r interval each step size holds on (bhrt_trace_core.h ray_iterate caches the size and its
     * interval per ray): the chain picks h_2_5 for r < t3, else h_5 for r < t2, else h_15 for
     * r < t1, else h_far -- for any order of the thresholds */
    {
        const double t1 = s->rs_x15, t2 = s->rs_x5, t3 = s->rs_x2_5;
        s->h_lo[3] = -INFINITY;
        s->h_hi[3] = t3;
        s->h_lo[2] = t3;
        s->h_hi[2] = t2;
        s->h_lo[1] = fmax(t2, t3);
        s->h_hi[1] = t1;
        s->h_lo[0] = fmax(t1, fmax(t2, t3));
        s->h_hi[0] = INFINITY;
    }
    {
        /* a step's nominal increment of state[2] is h * (a weighted sum of the constant
         * state[5] whose weights' magnitudes add up to <= 1.36, RKF45's 5th order; RK4 1) */
        const double hmax = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
        s->rot_vmax = hmax > 0.0 ? 0.78 / (hmax * 1.4) : INFINITY; /* 0.78 < pi/4 */
        if (!(s->rot_vmax >= 0.0)) s->rot_vmax = 0.0;              /* (NaN / Inf step sizes) */
    }
    s->max_dist = cfg->max_ray_distance;
    s->tol = cfg->tolerance;
    s->max_steps = cfg->max_integration_steps;
    s->method = (int)method;
    s->flags = flags;
    s->spin0 = bh->spin == 0.0;
    s->far_bounded = far_bounded(s);
    /* on the zero-acceleration paths an attempt's error is rounding alone, < 6e-15 of its scale
     * (proof at bhrt_trace_core.h rkf45_attempt): every attempt is accepted for tol >= 2^-30.
     * BHRT_ACCEPT_ALL=0 keeps the test (A/B) */
    s->accept_all = method == INTEGRATOR_RKF45 && s->tol >= 0x1p-30 && s->tol <= 0x1p300 &&
                    isfinite(s->h_2_5) && isfinite(s->h_5) && isfinite(s->h_15) &&
                    isfinite(s->h_far) && bhrt_env_int("BHRT_ACCEPT_ALL", 1) != 0;
    s->has_disk = dk != NULL;
    if (dk) {
        s->disk_in = dk->inner_radius;
        s->disk_out = dk->outer_radius;
        s->disk_tscale = dk->temperature_scale;
        s->disk_in_sq = sqrt_lower_bound(dk->inner_radius);
        s->disk_out_sq = sqrt_upper_bound(dk->outer_radius);
    }
    kp->refill = g_refill ? g_refill : refill_default(s);
    claim_policy(kp);
    kp->colour_fused = bhrt_colour_fused((int)method, dk != NULL, bh->spin != 0.0);
    kp->skip_redo = bhrt_env_int("BHRT_SKIP_REDO", 1) != 0;
    kp->block_lanes = bhrt_env_int("BHRT_TRACE_BLOCK", 256);
    kp->grid_div = bhrt_env_int("BHRT_GRID_DIV", 0);
    kp->grid_blocks = bhrt_env_int("BHRT_GRID_BLOCKS", 0);
    kp->min_tiles = bhrt_env_int("BHRT_MIN_TILES", 10);
    kp->cam.rows.row_block = 1;
    kp->cam.rows.num_shards = 1;
    return 0;
}

/* camera basis exactly as calculate_ray_direction forms it (raytracer.c:1013-1028), and
 * integrate_photon_path's origin-only set-up (raytracer.c:355-466, spacetime.c:15-33,
 * 201-237): every camera ray shares the origin, so its spherical coordinates, their sin/cos
 * and the metric there are computed once, here, with the same libm calls as the reference. */
void bhrt_fill_camera(bhrt_kparams* kp, const bhrt_camera* cam, int W, int H) {
    bhrt_camera_k* k = &kp->cam;
    double aspect = (double)W / (double)H;
    Vector3D fwd = vector3D_normalize(cam->direction);
    Vector3D right = vector3D_normalize(vector3D_cross(fwd, cam->up));
    Vector3D up = vector3D_cross(right, fwd);
    double fov_radians = cam->fov_deg * BH_PI / 180.0;
    double plane_h = 2.0 * tan(fov_radians / 2.0);
    kp->src = BHRT_SRC_CAMERA;
    k->fwd[0] = fwd.x; k->fwd[1] = fwd.y; k->fwd[2] = fwd.z;
    k->right[0] = right.x; k->right[1] = right.y; k->right[2] = right.z;
    k->up[0] = up.x; k->up[1] = up.y; k->up[2] = up.z;
    k->plane_h = plane_h;
    k->plane_w = plane_h * aspect;
    k->off_x = cam->use_offset ? cam->offset_x : 0.5;
    k->off_y = cam->use_offset ? cam->offset_y : 0.5;
    k->width = W;
    k->height = H;
    k->inv_width = 1.0 / (double)W;
    k->inv_block = 1.0 / (double)k->rows.row_block;
    bhrt_fill_origin(kp, &cam->position);
}

/* integrate_photon_path's origin-only set-up for rays that share `origin` (a camera frame, or
 * a ray array whose every origin is this one: shared_origin) */
void bhrt_fill_origin(bhrt_kparams* kp, const Vector3D* origin) {
    bhrt_camera_k* k = &kp->cam;
    k->pos[0] = origin->x;
    k->pos[1] = origin->y;
    k->pos[2] = origin->z;
    Vector3D sph;
    cartesian_to_spherical(origin, &sph);
    double r = sph.x, th = sph.y, ph = sph.z;
    double st = sin(th), ct = cos(th), sp = sin(ph), cp = cos(ph);
    k->r0 = r;
    k->th0 = th;
    k->ph0 = ph;
    k->st_cp = st * cp;
    k->st_sp = st * sp;
    k->ct = ct;
    k->ct_cp = ct * cp;
    k->ct_sp = ct * sp;
    k->st = st;
    k->neg_sp = -sp;
    k->cp = cp;
    k->r_st = r * st;
    k->st_tiny = fabs(st) < BH_EPSILON;
    SchwarzschildMetric m = calculate_schwarzschild_metric(r, &(BlackHoleParams){
        .schwarzschild_radius = kp->sc.rs});
    k->g_tt = m.g_tt;
    k->g_rr = m.g_rr;
    k->g_hh = m.g_thth;
    Vector3D p0;
    spherical_to_cartesian(&sph, &p0);
    k->p0[0] = p0.x;
    k->p0[1] = p0.y;
    k->p0[2] = p0.z;
    k->use_approx = r > kp->sc.rs_x15;
    /* the carried sin/cos of the origin's state angles start from the
     * reference's own libm values: state[2..3] = (th0, ph0) are st, ct, sp, cp above, and
     * state[1] = r0 is read as an angle by ray_derivatives */
    k->sp = sp;
    k->s_r0 = sin(r);
    k->c_r0 = cos(r);
    /* BHRT_ASSUME_NO_EVICT=1 (tests only): take the proof as given, so that a scene that does
     * evict shows what a wrong proof would do -- RAY_ERROR outputs and a harvest error */
    kp->no_evict = bhrt_env_int("BHRT_ASSUME_NO_EVICT", 0) ||
                   origin_no_evict(&kp->sc, r, th, ph, st, k->st_tiny, m.g_tt, m.g_rr, m.g_thth,
                                   k->use_approx);
}
