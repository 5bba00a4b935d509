/*
 * kerr.c -- physical geodesics: camera frames and ray arrays traced as true null geodesics of
 * Kerr in Kerr-Schild coordinates (the rule: include/bhrt_api.h "Physical geodesics"; the kernel:
 * kerr.hip k_kerr). An opt-in path beside the parity path: nothing here is reached by any other
 * entry point.
 *
 * A device call is its argument checks -- every refusal is decided before any HIP call -- and one
 * launch of k_kerr on the caller's stream, timed and counted like a trace launch: it takes a
 * control block of the context's ring through bhrt_ctx_launch_fn (the block's first word is the
 * kernel's claim counter, zero at launch like the rest), so it needs no scratch of its own and no
 * host wait. The host forms run the same launch into the context's cached device buffer and copy
 * back what was asked for.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the launcher named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <math.h>
#include <string.h>

#include "bhrt_host.h"
#include "kerr_init.h"

/* The checks below are shared with kerr_paths.c, kerr_rk45.c and kerr_emit.c through
 * bhrt_host.h, and so are the call struct, its filling and the host forms' staging further down. */
/* the scene's constants, or -1 with the error set; no HIP call */
int bhrt_kerr_scene(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, bhrt_kerr_k* k) {
    if (!bh || !cfg) {
        bhrt_set_err("kerr: blackhole and config must not be NULL");
        return -1;
    }
    if (!(fabs(bh->spin) < 1.0)) {
        bhrt_set_err("kerr: spin %g (|spin| < 1)", bh->spin);
        return -1;
    }
    if (!(isfinite(bh->mass) && bh->mass > 0.0)) {
        bhrt_set_err("kerr: mass %g (finite, > 0)", bh->mass);
        return -1;
    }
    if (!(isfinite(cfg->time_step) && cfg->time_step > 0.0)) {
        bhrt_set_err("kerr: time_step %g (finite, > 0)", cfg->time_step);
        return -1;
    }
    if (cfg->max_integration_steps < 0) {
        bhrt_set_err("kerr: max_integration_steps %d (>= 0)", cfg->max_integration_steps);
        return -1;
    }
    if (isnan(cfg->max_ray_distance)) {
        bhrt_set_err("kerr: max_ray_distance is NaN");
        return -1;
    }
    if (dk && !(dk->inner_radius >= 0.0 && dk->outer_radius >= 0.0)) {
        bhrt_set_err("kerr: disk radii %g, %g (not NaN, >= 0)", dk->inner_radius, dk->outer_radius);
        return -1;
    }
    memset(k, 0, sizeof *k);
    k->M = bh->mass;
    k->two_m = 2.0 * bh->mass;
    k->eight_m = 8.0 * bh->mass;
    k->a = -(bh->spin * bh->mass);
    k->a2 = k->a * k->a;
    k->r_plus = bh->mass + sqrt(bh->mass * bh->mass - k->a2);
    k->dt = cfg->time_step;
    k->max_dist = cfg->max_ray_distance;
    k->max_steps = cfg->max_integration_steps;
    k->has_disk = dk != NULL;
    if (dk) {
        k->disk_lo = dk->inner_radius * dk->inner_radius + k->a2;
        k->disk_hi = dk->outer_radius * dk->outer_radius + k->a2;
    }
    return 0;
}

int bhrt_kerr_out_bad(const bhrt_frame_soa* out, int flags) {
    if (!out) {
        bhrt_set_err("kerr: the output struct must not be NULL");
        return -1;
    }
    if (out->time_dilation) {
        bhrt_set_err("kerr: time_dilation is not produced (must be NULL)");
        return -1;
    }
    if ((out->rgb_r || out->rgb_g || out->rgb_b) && !(out->rgb_r && out->rgb_g && out->rgb_b)) {
        bhrt_set_err("kerr: rgb output needs all of rgb_r/g/b");
        return -1;
    }
    return bhrt_sky_check(flags, (flags & BHRT_FLAG_SKY) ? bhrt_current_device() : -1);
}

int bhrt_kerr_observer(const bhrt_kerr_k* k, const Vector3D* o, long i) {
    double f, l[3];
    if (bhrt_kerr_origin(o->x, o->y, o->z, k->a, k->a2, k->two_m, k->r_plus, &f, l)) return 0;
    if (i < 0)
        bhrt_set_err("kerr: no static observer at the origin (%g, %g, %g): f = %g", o->x, o->y,
                     o->z, f);
    else
        bhrt_set_err("kerr: no static observer at the origin of ray %ld (%g, %g, %g): f = %g", i,
                     o->x, o->y, o->z, f);
    return -1;
}

int bhrt_kerr_frame_check(const char* who, const bhrt_camera* cam, int W, int H,
                          const bhrt_rows* rows, int* nrows) {
    if (!cam) {
        bhrt_set_err("%s: camera must not be NULL", who);
        return -1;
    }
    if (W < 1 || H < 1) {
        bhrt_set_err("%s: invalid size %d x %d", who, W, H);
        return -1;
    }
    *nrows = bhrt_shard_rows(H, rows);
    if (*nrows < 0 || (long)*nrows * W > 0x7fffffffL) {
        bhrt_set_err("%s: invalid row sharding or frame too large (%d x %d)", who, W, H);
        return -1;
    }
    return 0;
}

/* a camera call's checks: 0 and the shard's rows, or -1 */
static int kerr_frame_check(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                            bhrt_kerr_k* k, int* nrows) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || bhrt_kerr_out_bad(out, flags) ||
        bhrt_kerr_frame_check("kerr", cam, W, H, rows, nrows))
        return -1;
    return bhrt_kerr_observer(k, &cam->position, -1);
}

int bhrt_kerr_rays_check(const Ray* rays, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                         const bhrt_frame_soa* out, bhrt_kerr_k* k) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || bhrt_kerr_out_bad(out, flags)) return -1;
    if (n <= 0) {
        bhrt_set_err("kerr: n = %d rays (at least 1)", n);
        return -1;
    }
    if (!rays) {
        bhrt_set_err("kerr: rays must not be NULL");
        return -1;
    }
    return 0;
}

static int kerr_fn(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0, void* ev1) {
    return bhrt_launch_kerr(kp, (const bhrt_kerr_k*)arg, stream, ev0, ev1);
}

int bhrt_kerr_fill(const bhrt_kerr_call* a, bhrt_kparams* kp, bhrt_kerr_k* k) {
    /* the colour's constants and the sky map (the integration's are a->k) */
    if (bhrt_fill_scene(kp, a->bh, a->dk, a->cfg, INTEGRATOR_RK4, a->flags)) return -1;
    *k = *a->k;
    if (a->cam) {
        bhrt_fill_camera(kp, a->cam, a->W, a->H);
        if (a->rows && a->rows->num_shards > 1) kp->cam.rows = *a->rows;
        kp->n = a->nrows * a->W;
        k->nrows = a->nrows;
        k->tiles_x = (a->W + 7) / 8;
        k->ntiles = k->tiles_x * ((a->nrows + 7) / 8);
    } else {
        kp->src = BHRT_SRC_RAYS;
        kp->rays = a->d_rays;
        kp->n = a->n;
    }
    kp->out = *a->out;
    k->h_residual = a->h_residual;
    k->lz_drift = a->lz_drift;
    return 0;
}

/* the launch on `st` of context c (c NULL: the current device's, made here); device pointers */
static int kerr_body(devctx_t* c, hipStream_t st, const void* arg) {
    const bhrt_kerr_call* a = (const bhrt_kerr_call*)arg;
    if (!c) c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    bhrt_kparams kp;
    bhrt_kerr_k k;
    if (bhrt_kerr_fill(a, &kp, &k)) return -1;
    return bhrt_ctx_launch_fn(c, &kp, st, kerr_fn, &k);
}

int bhrt_kerr_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                           const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                           const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                           const bhrt_kerr_diag* diag, void* stream) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (kerr_frame_check(bh, dk, cfg, cam, W, H, rows, flags, out, &k, &nrows)) return -1;
    if (nrows == 0) return 0;
    const bhrt_kerr_call a = {bh, dk, cfg, cam, W, H, nrows, rows, NULL, 0, flags, out,
                              diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, kerr_body, &a);
}

int bhrt_kerr_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                          const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                          const bhrt_frame_soa* out, const bhrt_kerr_diag* diag, void* stream) {
    bhrt_kerr_k k;
    if (bhrt_kerr_rays_check(d_rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    const bhrt_kerr_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, d_rays, n, flags, out,
                              diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, kerr_body, &a);
}

int bhrt_kerr_rays_on_device(devctx_t* c, hipStream_t st, const Ray* d_rays, int n,
                             const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, int flags, const bhrt_frame_soa* out,
                             const bhrt_kerr_diag* diag, const bhrt_kerr_k* k) {
    const bhrt_kerr_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, d_rays, n, flags, out,
                              diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, k};
    return kerr_body(c, st, &a);
}

size_t bhrt_kerr_stage_bytes(const bhrt_frame_soa* hout, long n, const bhrt_kerr_plane* pl,
                             int npl) {
    size_t bytes = bhrt_soa_bytes(hout, n);
    for (int i = 0; i < npl; i++) bytes += align256(pl[i].bytes);
    return bytes;
}

int bhrt_kerr_stage_carve(char** p, hipStream_t st, const bhrt_frame_soa* hout, long n,
                          bhrt_frame_soa* dout, const bhrt_kerr_plane* pl, int npl) {
    const size_t N = (size_t)n;
    bhrt_soa_carve(p, hout, n, dout);
    for (int i = 0; i < npl; i++) { /* (a plane not asked for keeps its place: the slot is NULL) */
        void* const d = pl[i].host ? (void*)*p : NULL;
        memcpy(pl[i].dev, &d, sizeof d);
        *p += align256(pl[i].bytes);
    }
    /* sky_* are written for RAY_MAX_DISTANCE rays alone, and a `preload` plane in part: the other
     * elements of the caller's arrays keep what they held, so the device planes start from the
     * caller's values */
    double* const hsky[3] = {hout->sky_x, hout->sky_y, hout->sky_z};
    double* const dsky[3] = {dout->sky_x, dout->sky_y, dout->sky_z};
    for (int f = 0; f < 3; f++)
        if (hsky[f]) HIP_TRY(hipMemcpyAsync(dsky[f], hsky[f], 8 * N, hipMemcpyHostToDevice, st));
    for (int i = 0; i < npl; i++)
        if (pl[i].host && pl[i].preload) {
            void* d;
            memcpy(&d, pl[i].dev, sizeof d);
            HIP_TRY(hipMemcpyAsync(d, pl[i].host, pl[i].bytes, hipMemcpyHostToDevice, st));
        }
    return 0;
}

int bhrt_kerr_stage_back(const bhrt_frame_soa* hout, long n, const bhrt_frame_soa* dout,
                         const bhrt_kerr_plane* pl, int npl) {
    /* plain synchronous copies: caller memory is never page-locked */
    void* const* hh = (void* const*)hout;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (hh[f])
            HIP_TRY(hipMemcpy(hh[f], ((void* const*)dout)[f], k_fsize[f] * (size_t)n,
                              hipMemcpyDeviceToHost));
    for (int i = 0; i < npl; i++)
        if (pl[i].host) {
            void* d;
            memcpy(&d, pl[i].dev, sizeof d);
            HIP_TRY(hipMemcpy(pl[i].host, d, pl[i].bytes, hipMemcpyDeviceToHost));
        }
    return 0;
}

int bhrt_kerr_host(bhrt_kerr_call* a, const Ray* rays, long n, const bhrt_kerr_plane* pl, int npl,
                   bhrt_stream_body body, const void* arg) {
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    hipStream_t st = c->stream;
    const size_t N = (size_t)n;
    const bhrt_frame_soa* hout = a->out;
    size_t bytes = bhrt_kerr_stage_bytes(hout, n, pl, npl);
    if (rays) bytes += align256(N * sizeof(Ray));
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes, 0)) return -1;
    char* p = (char*)c->d_ss;
    if (rays) {
        a->d_rays = (const Ray*)p;
        HIP_TRY(hipMemcpyAsync(p, rays, N * sizeof(Ray), hipMemcpyHostToDevice, st));
        p += align256(N * sizeof(Ray));
    }
    bhrt_frame_soa dout;
    if (bhrt_kerr_stage_carve(&p, st, hout, n, &dout, pl, npl)) return -1;
    a->out = &dout;
    if (body(c, st, arg)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    return bhrt_kerr_stage_back(hout, n, &dout, pl, npl);
}

/* the host forms: `a` with the host out and host rays (or a camera), n rays in all; the
 * diagnostics are its two planes */
static int kerr_host(bhrt_kerr_call* a, const bhrt_kerr_diag* diag, const Ray* rays, long n) {
    const size_t N = (size_t)n;
    const bhrt_kerr_plane pl[] = {{diag ? diag->h_residual : NULL, &a->h_residual, 8 * N, 0},
                                  {diag ? diag->lz_drift : NULL, &a->lz_drift, 8 * N, 0}};
    return bhrt_kerr_host(a, rays, n, pl, 2, kerr_body, a);
}

int bhrt_kerr_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H, int flags,
                    const bhrt_frame_soa* out, const bhrt_kerr_diag* diag) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (kerr_frame_check(bh, dk, cfg, cam, W, H, NULL, flags, out, &k, &nrows)) return -1;
    bhrt_kerr_call a = {bh, dk, cfg, cam, W, H, nrows, NULL, NULL, 0, flags, out,
                        NULL, NULL, &k};
    return kerr_host(&a, diag, NULL, (long)nrows * W);
}

int bhrt_kerr_rays(const Ray* rays, int n, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                   const SimulationConfig* cfg, int flags, const bhrt_frame_soa* out,
                   const bhrt_kerr_diag* diag) {
    bhrt_kerr_k k;
    if (bhrt_kerr_rays_check(rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    bhrt_kerr_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, NULL, n, flags, out,
                        NULL, NULL, &k};
    return kerr_host(&a, diag, rays, n);
}

int bhrt_kerr_ray_init(const BlackHoleParams* bh, const Vector3D* origin, const Vector3D* direction,
                       double state[6], double* E) {
    if (!bh || !origin || !direction || !state || !E) {
        bhrt_set_err("kerr: NULL argument");
        return -1;
    }
    const SimulationConfig cfg = {.time_step = 1.0};
    bhrt_kerr_k k;
    if (bhrt_kerr_scene(bh, NULL, &cfg, &k) || bhrt_kerr_observer(&k, origin, -1)) return -1;
    const double d[3] = {direction->x, direction->y, direction->z};
    double n[3], l[3], p[3], f;
    bhrt_kerr_unit(d, n);
    (void)bhrt_kerr_origin(origin->x, origin->y, origin->z, k.a, k.a2, k.two_m, k.r_plus, &f, l);
    bhrt_kerr_photon(f, l, n, p, E);
    state[0] = origin->x;
    state[1] = origin->y;
    state[2] = origin->z;
    state[3] = p[0];
    state[4] = p[1];
    state[5] = p[2];
    return 0;
}

/* the scene's constants with the particle rule's spin a = +(spin * mass), or -1 */
static int particle_scene(const BlackHoleParams* bh, bhrt_kerr_k* k) {
    const SimulationConfig cfg = {.time_step = 1.0};
    if (bhrt_kerr_scene(bh, NULL, &cfg, k)) return -1;
    k->a = bh->spin * bh->mass;
    return 0;
}

int bhrt_kerr_particle_state(const BlackHoleParams* bh, const Vector3D* position,
                             const Vector3D* velocity, double state[6], double* E, double* ut) {
    if (!bh || !position || !velocity || !state || !E || !ut) {
        bhrt_set_err("kerr particles: NULL argument");
        return -1;
    }
    bhrt_kerr_k k;
    if (particle_scene(bh, &k)) return -1;
    const double v[3] = {velocity->x, velocity->y, velocity->z};
    double f, l[3], p[3], e, u;
    const double r = bhrt_kerr_fields(position->x, position->y, position->z, k.a, k.a2, k.two_m,
                                      &f, l);
    if (r <= k.r_plus || !bhrt_kerr_particle(f, l, v, p, &e, &u)) return 1;
    state[0] = position->x;
    state[1] = position->y;
    state[2] = position->z;
    state[3] = p[0];
    state[4] = p[1];
    state[5] = p[2];
    *E = e;
    *ut = u;
    return 0;
}

int bhrt_kerr_orbit_velocity(const BlackHoleParams* bh, const Vector3D* position, int prograde,
                             Vector3D* velocity) {
    if (!bh || !position || !velocity) {
        bhrt_set_err("kerr particles: NULL argument");
        return -1;
    }
    bhrt_kerr_k k;
    if (particle_scene(bh, &k)) return -1;
    if (!(position->z == 0.0)) {
        bhrt_set_err("kerr particles: an equatorial orbit needs z == 0 (z = %g)", position->z);
        return -1;
    }
    const double x = position->x, y = position->y;
    const double s = prograde ? 1.0 : -1.0;
    const double r = sqrt((x * x + y * y) - k.a2);
    const double sm = sqrt(k.M), sr = sqrt(r);
    if (!(r > k.r_plus) || !((r * sr - 3.0 * k.M * sr) + s * (2.0 * k.a * sm) > 0.0)) return 1;
    const double omega = s * sm / (r * sr + s * (k.a * sm));
    velocity->x = omega * -y;
    velocity->y = omega * x;
    velocity->z = 0.0;
    return 0;
}
