/*
 * kerr_rk45.c -- physical geodesics with adaptive steps: camera frames and ray arrays traced by
 * Dormand-Prince 5(4) attempts under config->tolerance (the rule: include/bhrt_api.h "Physical
 * geodesics, adaptive steps"; the kernel: kerr.hip k_kerr_rk45). An opt-in path beside
 * bhrt_kerr_*: nothing here is reached by any other entry point.
 *
 * The calls are kerr.c's in shape: the argument checks -- kerr.c's own, shared through
 * bhrt_host.h, and the tolerance's; every refusal is decided before any HIP call -- and one launch
 * on the caller's stream through bhrt_ctx_launch_fn, timed and counted like a trace launch
 * (iterations: attempts). The host forms run the same launch into the context's cached device
 * buffer and copy back what was asked for; `rejected` is one more plane.
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

/* a camera call's checks (kerr.c's kerr_frame_check and the tolerance): 0 and the shard's rows */
static int rk45_frame_check(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                            bhrt_kerr_k* k, int* nrows) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || rk45_tol_bad(cfg) || bhrt_kerr_out_bad(out, flags))
        return -1;
    if (!cam) {
        bhrt_set_err("kerr_rk45: camera must not be NULL");
        return -1;
    }
    if (W < 1 || H < 1) {
        bhrt_set_err("kerr_rk45: invalid size %d x %d", W, H);
        return -1;
    }
    *nrows = bhrt_shard_rows(H, rows);
    if (*nrows < 0 || (long)*nrows * W > 0x7fffffffL) {
        bhrt_set_err("kerr_rk45: invalid row sharding or frame too large (%d x %d)", W, H);
        return -1;
    }
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
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam; /* NULL: a ray array */
    int W, H, nrows;
    const bhrt_rows* rows;
    const Ray* d_rays;
    int n;
    int flags;
    const bhrt_frame_soa* out;
    const bhrt_kerr_rk45_diag* diag;
    const bhrt_kerr_k* k;
} rk45_call;

/* the launch on `st` of context c (c NULL: the current device's, made here); device pointers */
static int rk45_body(devctx_t* c, hipStream_t st, const void* arg) {
    const rk45_call* a = (const rk45_call*)arg;
    if (!c) c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    bhrt_kparams kp;
    /* the colour's constants and the sky map (the integration's are a->k) */
    if (bhrt_fill_scene(&kp, a->bh, a->dk, a->cfg, INTEGRATOR_RK4, a->flags)) return -1;
    bhrt_kerr_rk45_k rk;
    memset(&rk, 0, sizeof rk);
    rk.k = *a->k;
    rk.tol = a->cfg->tolerance;
    if (a->cam) {
        bhrt_fill_camera(&kp, a->cam, a->W, a->H);
        if (a->rows && a->rows->num_shards > 1) kp.cam.rows = *a->rows;
        kp.n = a->nrows * a->W;
        rk.k.nrows = a->nrows;
        rk.k.tiles_x = (a->W + 7) / 8;
        rk.k.ntiles = rk.k.tiles_x * ((a->nrows + 7) / 8);
    } else {
        kp.src = BHRT_SRC_RAYS;
        kp.rays = a->d_rays;
        kp.n = a->n;
    }
    kp.out = *a->out;
    if (a->diag) {
        rk.k.h_residual = a->diag->h_residual;
        rk.k.lz_drift = a->diag->lz_drift;
        rk.rejected = a->diag->rejected;
    }
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
    const rk45_call a = {bh, dk, cfg, cam, W, H, nrows, rows, NULL, 0, flags, out, diag, &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, rk45_body, &a);
}

int bhrt_kerr_rk45_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                               const AccretionDiskParams* dk, const SimulationConfig* cfg,
                               int flags, const bhrt_frame_soa* out,
                               const bhrt_kerr_rk45_diag* diag, void* stream) {
    bhrt_kerr_k k;
    if (rk45_rays_check(d_rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    const rk45_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, d_rays, n, flags, out, diag, &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, rk45_body, &a);
}

/* the host forms: `a` with host out / diag and host rays (or a camera); n rays in all */
static int rk45_host(rk45_call* a, const Ray* rays, long n) {
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    hipStream_t st = c->stream;
    const size_t N = (size_t)n;
    const bhrt_frame_soa* hout = a->out;
    const bhrt_kerr_rk45_diag* hdiag = a->diag;
    size_t bytes = bhrt_soa_bytes(hout, n) + 2 * align256(8 * N) + align256(4 * N);
    if (rays) bytes += align256(N * sizeof(Ray));
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes, 0)) return -1;
    char* p = (char*)c->d_ss;
    if (rays) {
        a->d_rays = (const Ray*)p;
        HIP_TRY(hipMemcpyAsync(p, rays, N * sizeof(Ray), hipMemcpyHostToDevice, st));
        p += align256(N * sizeof(Ray));
    }
    bhrt_frame_soa dout;
    bhrt_soa_carve(&p, hout, n, &dout);
    bhrt_kerr_rk45_diag ddiag = {NULL, NULL, NULL};
    if (hdiag && hdiag->h_residual) ddiag.h_residual = (double*)p;
    p += align256(8 * N);
    if (hdiag && hdiag->lz_drift) ddiag.lz_drift = (double*)p;
    p += align256(8 * N);
    if (hdiag && hdiag->rejected) ddiag.rejected = (int*)p;
    a->out = &dout;
    a->diag = &ddiag;
    /* sky_* are written for RAY_MAX_DISTANCE rays alone: the other elements of the caller's
     * arrays keep what they held, so the device planes start from the caller's values */
    double* const hsky[3] = {hout->sky_x, hout->sky_y, hout->sky_z};
    double* const dsky[3] = {dout.sky_x, dout.sky_y, dout.sky_z};
    for (int f = 0; f < 3; f++)
        if (hsky[f]) HIP_TRY(hipMemcpyAsync(dsky[f], hsky[f], 8 * N, hipMemcpyHostToDevice, st));
    if (rk45_body(c, st, a)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    /* plain synchronous copies: caller memory is never page-locked */
    void* const* hh = (void* const*)hout;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (hh[f])
            HIP_TRY(hipMemcpy(hh[f], ((void**)&dout)[f], k_fsize[f] * N, hipMemcpyDeviceToHost));
    if (ddiag.h_residual)
        HIP_TRY(hipMemcpy(hdiag->h_residual, ddiag.h_residual, 8 * N, hipMemcpyDeviceToHost));
    if (ddiag.lz_drift)
        HIP_TRY(hipMemcpy(hdiag->lz_drift, ddiag.lz_drift, 8 * N, hipMemcpyDeviceToHost));
    if (ddiag.rejected)
        HIP_TRY(hipMemcpy(hdiag->rejected, ddiag.rejected, 4 * N, hipMemcpyDeviceToHost));
    return 0;
}

int bhrt_kerr_rk45_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         int flags, const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (rk45_frame_check(bh, dk, cfg, cam, W, H, NULL, flags, out, &k, &nrows)) return -1;
    rk45_call a = {bh, dk, cfg, cam, W, H, nrows, NULL, NULL, 0, flags, out, diag, &k};
    return rk45_host(&a, NULL, (long)nrows * W);
}

int bhrt_kerr_rk45_rays(const Ray* rays, int n, const BlackHoleParams* bh,
                        const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                        const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag) {
    bhrt_kerr_k k;
    if (rk45_rays_check(rays, n, bh, dk, cfg, flags, out, &k)) return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    rk45_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, NULL, n, flags, out, diag, &k};
    return rk45_host(&a, rays, n);
}
