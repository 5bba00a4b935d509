/*
 * kerr_rk45.c -- physical geodesics with adaptive steps: camera frames and ray arrays traced by
 * Dormand-Prince 5(4) attempts under config->tolerance (the rule: include/bhrt_api.h "Physical
 * geodesics, adaptive steps"; the kernel: kerr.hip k_kerr_rk45). An opt-in path beside
 * bhrt_kerr_*: nothing here is reached by any other entry point.
 *
 * The calls are kerr.c's in shape: the argument checks -- kerr.c's own, shared through
 * bhrt_host.h, and the tolerance's; every refusal is decided before any HIP call -- and one launch
 * on the caller's stream through bhrt_ctx_launch_fn, timed and counted like a trace launch
 * (iterations: attempts). The call struct's shared part, the filling of the launch's arguments
 * and the host forms' staging are kerr.c's too (bhrt_kerr_call, bhrt_kerr_fill, bhrt_kerr_host);
 * this file adds the tolerance and `rejected`, one more plane.
 *
 * A file of its own (the Makefile's HOST_FEATURE): it names its own launcher and no other.
 */
#define _GNU_SOURCE
#include <math.h>
#include <string.h>

#include "bhrt_host.h"

/* the tolerance's refusal; no HIP call */
static int rk45_tol_bad(const SimulationConfig* cfg) {
    if (isfinite(cfg->tolerance) && cfg->tolerance >= 1e-12 && cfg->tolerance <= 1e-2) return 0;
    bhrt_set_err("kerr_rk45: tolerance %g (finite, within [1e-12, 1e-2])", cfg->tolerance);
    return -1;
}

/* a camera call's checks (kerr.c's and the tolerance): 0 and the shard's rows */
static int rk45_frame_check(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                            bhrt_kerr_k* k, int* nrows) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || rk45_tol_bad(cfg) || bhrt_kerr_out_bad(out, flags) ||
        bhrt_kerr_frame_check("kerr_rk45", cam, W, H, rows, nrows))
        return -1;
    return bhrt_kerr_observer(k, &cam->position, -1);
}

static int rk45_rays_check(const Ray* rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                           const bhrt_frame_soa* out, bhrt_kerr_k* k) {
    /* (a NULL config is refused before its tolerance is read) */
    return bhrt_kerr_rays_check(rays, n, bh, dk, cfg, flags, out, k) || rk45_tol_bad(cfg) ? -1 : 0;
}

static int rk45_fn(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0, void* ev1) {
    return bhrt_launch_kerr_rk45(kp, (const bhrt_kerr_rk45_k*)arg, stream, ev0, ev1);
}

typedef struct { /* one checked launch, for its run under the stream rule */
    bhrt_kerr_call c;
    int* rejected; /* bhrt_kerr_rk45_diag's third plane or NULL */
} rk45_call;

/* the launch on `st` of context c (c NULL: the current device's, made here); device pointers */
static int rk45_body(devctx_t* c, hipStream_t st, const void* arg) {
    const rk45_call* a = (const rk45_call*)arg;
    if (!c) c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    bhrt_kparams kp;
    bhrt_kerr_rk45_k rk;
    memset(&rk, 0, sizeof rk);
    if (bhrt_kerr_fill(&a->c, &kp, &rk.k)) return -1;
    rk.tol = a->c.cfg->tolerance;
    rk.rejected = a->rejected;
    return bhrt_ctx_launch_fn(c, &kp, st, rk45_fn, &rk);
}

int bhrt_kerr_rk45_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                                const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                                const bhrt_kerr_rk45_diag* diag, void* stream) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (rk45_frame_check(bh, dk, cfg, cam, W, H, rows, flags, out, &k, &nrows)) return -1;
    if (nrows == 0) return 0;
    const rk45_call a = {{bh, dk, cfg, cam, W, H, nrows, rows, NULL, 0, flags, out,
                          diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k},
                         diag ? diag->rejected : NULL};
    return bhrt_on_stream(NULL, (hipStream_t)stream, rk45_body, &a);
}

int bhrt_kerr_rk45_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                               const AccretionDiskParams* dk, const SimulationConfig* cfg,
                               int flags, const bhrt_frame_soa* out,
                               const bhrt_kerr_rk45_diag* diag, void* stream) {
    bhrt_kerr_k k;
    if (rk45_rays_check(d_rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    const rk45_call a = {{bh, dk, cfg, NULL, 0, 0, 0, NULL, d_rays, n, flags, out,
                          diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k},
                         diag ? diag->rejected : NULL};
    return bhrt_on_stream(NULL, (hipStream_t)stream, rk45_body, &a);
}

/* the host forms: `a` with the host out and host rays (or a camera), n rays in all; the
 * diagnostics are its three planes */
static int rk45_host(rk45_call* a, const bhrt_kerr_rk45_diag* diag, const Ray* rays, long n) {
    const size_t N = (size_t)n;
    const bhrt_kerr_plane pl[] = {{diag ? diag->h_residual : NULL, &a->c.h_residual, 8 * N, 0},
                                  {diag ? diag->lz_drift : NULL, &a->c.lz_drift, 8 * N, 0},
                                  {diag ? diag->rejected : NULL, &a->rejected, 4 * N, 0}};
    return bhrt_kerr_host(&a->c, rays, n, pl, 3, rk45_body, a);
}

int bhrt_kerr_rk45_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         int flags, const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (rk45_frame_check(bh, dk, cfg, cam, W, H, NULL, flags, out, &k, &nrows)) return -1;
    rk45_call a = {{bh, dk, cfg, cam, W, H, nrows, NULL, NULL, 0, flags, out, NULL, NULL, &k},
                   NULL};
    return rk45_host(&a, diag, NULL, (long)nrows * W);
}

int bhrt_kerr_rk45_rays(const Ray* rays, int n, const BlackHoleParams* bh,
                        const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                        const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag) {
    bhrt_kerr_k k;
    if (rk45_rays_check(rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    rk45_call a = {{bh, dk, cfg, NULL, 0, 0, 0, NULL, NULL, n, flags, out, NULL, NULL, &k},
                   NULL};
    return rk45_host(&a, diag, rays, n);
}
