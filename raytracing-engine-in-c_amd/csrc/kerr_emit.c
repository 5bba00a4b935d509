/*
 * kerr_emit.c -- Kerr disk emission: camera frames and ray arrays traced by the adaptive rule with
 * up to K recorded disk crossings per ray, each with its redshift factor, and the intensity built
 * from them (the rule: include/bhrt_api.h "Kerr disk emission"; the kernel: kerr.hip k_kerr_emit;
 * the redshift's arithmetic: kerr_emit.h). An opt-in path beside bhrt_kerr_rk45_*: nothing here is
 * reached by any other entry point.
 *
 * The calls are kerr_rk45.c's in shape: the argument checks -- kerr.c's own, shared through
 * bhrt_host.h, the tolerance's and the emission's; every refusal is decided before any HIP call --
 * and one launch on the caller's stream through bhrt_ctx_launch_fn, timed and counted like a trace
 * launch (iterations: attempts). The host forms run the same launch into the context's cached
 * device buffer and copy back what was asked for. radius and redshift elements beyond a ray's
 * count are not written, so their device planes start from the caller's values.
 *
 * A file of its own (the Makefile's HOST_FEATURE): it names its own launcher and no other.
 */
#define _GNU_SOURCE
#include <limits.h>
#include <math.h>
#include <string.h>

#include "bhrt_host.h"
#include "kerr_emit.h"

/* the refusals this family adds to the adaptive calls' (n: the rays of the call); no HIP call */
static int emit_bad(const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                    const bhrt_frame_soa* out, const bhrt_kerr_emit_params* ep,
                    const bhrt_kerr_emit_out* eo, long n) {
    if (!(isfinite(cfg->tolerance) && cfg->tolerance >= 1e-12 && cfg->tolerance <= 1e-2)) {
        bhrt_set_err("kerr_emit: tolerance %g (finite, within [1e-12, 1e-2])", cfg->tolerance);
        return -1;
    }
    if (!dk) {
        bhrt_set_err("kerr_emit: disk must not be NULL");
        return -1;
    }
    if (!ep) {
        bhrt_set_err("kerr_emit: params must not be NULL");
        return -1;
    }
    if (ep->max_crossings < 1 || ep->max_crossings > BHRT_EMIT_MAX_CROSSINGS) {
        bhrt_set_err("kerr_emit: max_crossings %d (1..%d)", ep->max_crossings,
                     BHRT_EMIT_MAX_CROSSINGS);
        return -1;
    }
    if (!(isfinite(ep->emissivity_index) && ep->emissivity_index >= 0.0)) {
        bhrt_set_err("kerr_emit: emissivity_index %g (finite, >= 0)", ep->emissivity_index);
        return -1;
    }
    if (!(isfinite(ep->gain) && ep->gain >= 0.0)) {
        bhrt_set_err("kerr_emit: gain %g (finite, >= 0)", ep->gain);
        return -1;
    }
    if (flags & BHRT_FLAG_DOPPLER) {
        bhrt_set_err("kerr_emit: BHRT_FLAG_DOPPLER is not taken (the redshift factor replaces it)");
        return -1;
    }
    int any = eo && (eo->count || eo->radius || eo->redshift || eo->intensity);
    void* const* f = (void* const*)out;
    for (int i = 0; i < BHRT_NFIELDS; i++) any = any || f[i] != NULL;
    if (!any) {
        bhrt_set_err("kerr_emit: no output at all");
        return -1;
    }
    if ((long)ep->max_crossings * n > (long)INT_MAX) {
        bhrt_set_err("kerr_emit: max_crossings * n = %ld elements (at most INT_MAX)",
                     (long)ep->max_crossings * n);
        return -1;
    }
    return 0;
}

/* a camera call's checks (kerr_rk45.c's and the emission's): 0 and the shard's rows */
static int emit_frame_check(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                            const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo,
                            bhrt_kerr_k* k, int* nrows) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || bhrt_kerr_out_bad(out, flags)) return -1;
    if (!cam) {
        bhrt_set_err("kerr_emit: camera must not be NULL");
        return -1;
    }
    if (W < 1 || H < 1) {
        bhrt_set_err("kerr_emit: invalid size %d x %d", W, H);
        return -1;
    }
    *nrows = bhrt_shard_rows(H, rows);
    if (*nrows < 0 || (long)*nrows * W > 0x7fffffffL) {
        bhrt_set_err("kerr_emit: invalid row sharding or frame too large (%d x %d)", W, H);
        return -1;
    }
    if (emit_bad(dk, cfg, flags, out, ep, eo, (long)*nrows * W)) return -1;
    return bhrt_kerr_observer(k, &cam->position, -1);
}

static int emit_rays_check(const Ray* rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                           const bhrt_frame_soa* out, const bhrt_kerr_emit_params* ep,
                           const bhrt_kerr_emit_out* eo, bhrt_kerr_k* k) {
    return bhrt_kerr_rays_check(rays, n, bh, dk, cfg, flags, out, k) ||
                   emit_bad(dk, cfg, flags, out, ep, eo, n)
               ? -1
               : 0;
}

static int emit_fn(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0, void* ev1) {
    return bhrt_launch_kerr_emit(kp, (const bhrt_kerr_emit_k*)arg, stream, ev0, ev1);
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
    const bhrt_kerr_emit_params* ep;
    const bhrt_kerr_emit_out* eo;
    const bhrt_kerr_k* k;
} emit_call;

/* the launch on `st` of context c (c NULL: the current device's, made here); device pointers */
static int emit_body(devctx_t* c, hipStream_t st, const void* arg) {
    const emit_call* a = (const emit_call*)arg;
    if (!c) c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    bhrt_kparams kp;
    /* the colour's constants and the sky map (the integration's are a->k) */
    if (bhrt_fill_scene(&kp, a->bh, a->dk, a->cfg, INTEGRATOR_RK4, a->flags)) return -1;
    bhrt_kerr_emit_k ek;
    memset(&ek, 0, sizeof ek);
    ek.rk.k = *a->k;
    ek.rk.tol = a->cfg->tolerance;
    ek.max_crossings = a->ep->max_crossings;
    ek.q = a->ep->emissivity_index;
    ek.gain = a->ep->gain;
    ek.spin_a = a->bh->spin * a->bh->mass;
    if (a->eo) ek.out = *a->eo;
    if (a->cam) {
        bhrt_fill_camera(&kp, a->cam, a->W, a->H);
        if (a->rows && a->rows->num_shards > 1) kp.cam.rows = *a->rows;
        kp.n = a->nrows * a->W;
        ek.rk.k.nrows = a->nrows;
        ek.rk.k.tiles_x = (a->W + 7) / 8;
        ek.rk.k.ntiles = ek.rk.k.tiles_x * ((a->nrows + 7) / 8);
    } else {
        kp.src = BHRT_SRC_RAYS;
        kp.rays = a->d_rays;
        kp.n = a->n;
    }
    kp.out = *a->out;
    if (a->diag) {
        ek.rk.k.h_residual = a->diag->h_residual;
        ek.rk.k.lz_drift = a->diag->lz_drift;
        ek.rk.rejected = a->diag->rejected;
    }
    return bhrt_ctx_launch_fn(c, &kp, st, emit_fn, &ek);
}

int bhrt_kerr_emit_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                                const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                                const bhrt_kerr_rk45_diag* diag, const bhrt_kerr_emit_params* ep,
                                const bhrt_kerr_emit_out* eo, void* stream) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (emit_frame_check(bh, dk, cfg, cam, W, H, rows, flags, out, ep, eo, &k, &nrows)) return -1;
    if (nrows == 0) return 0;
    const emit_call a = {bh,   dk,    cfg, cam,  W,  H,  nrows, rows,
                         NULL, 0,     flags, out, diag, ep, eo,    &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, emit_body, &a);
}

int bhrt_kerr_emit_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                               const AccretionDiskParams* dk, const SimulationConfig* cfg,
                               int flags, const bhrt_frame_soa* out,
                               const bhrt_kerr_rk45_diag* diag, const bhrt_kerr_emit_params* ep,
                               const bhrt_kerr_emit_out* eo, void* stream) {
    bhrt_kerr_k k;
    if (emit_rays_check(d_rays, n, bh, dk, cfg, flags, out, ep, eo, &k)) return -1;
    const emit_call a = {bh,     dk, cfg,   NULL, 0,    0,  0,  NULL,
                         d_rays, n,  flags, out,  diag, ep, eo, &k};
    return bhrt_on_stream(NULL, (hipStream_t)stream, emit_body, &a);
}

/* the host forms: `a` with host out / diag / emit and host rays (or a camera); n rays in all */
static int emit_host(emit_call* a, const Ray* rays, long n) {
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    hipStream_t st = c->stream;
    const size_t N = (size_t)n, K = (size_t)a->ep->max_crossings;
    const bhrt_frame_soa* hout = a->out;
    const bhrt_kerr_rk45_diag* hdiag = a->diag;
    const bhrt_kerr_emit_out* heo = a->eo;
    size_t bytes = bhrt_soa_bytes(hout, n) + 2 * align256(8 * N) + align256(4 * N) /* diag */
                   + align256(4 * N) + 2 * align256(8 * K * N) + align256(8 * N); /* emit */
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
    p += align256(4 * N);
    bhrt_kerr_emit_out deo = {NULL, NULL, NULL, NULL};
    if (heo && heo->count) deo.count = (int*)p;
    p += align256(4 * N);
    if (heo && heo->radius) deo.radius = (double*)p;
    p += align256(8 * K * N);
    if (heo && heo->redshift) deo.redshift = (double*)p;
    p += align256(8 * K * N);
    if (heo && heo->intensity) deo.intensity = (double*)p;
    a->out = &dout;
    a->diag = &ddiag;
    a->eo = &deo;
    /* sky_* are written for RAY_MAX_DISTANCE rays alone, radius and redshift below a ray's count
     * alone: the other elements of the caller's arrays keep what they held, so the device planes
     * start from the caller's values */
    double* const hsky[3] = {hout->sky_x, hout->sky_y, hout->sky_z};
    double* const dsky[3] = {dout.sky_x, dout.sky_y, dout.sky_z};
    for (int f = 0; f < 3; f++)
        if (hsky[f]) HIP_TRY(hipMemcpyAsync(dsky[f], hsky[f], 8 * N, hipMemcpyHostToDevice, st));
    if (deo.radius)
        HIP_TRY(hipMemcpyAsync(deo.radius, heo->radius, 8 * K * N, hipMemcpyHostToDevice, st));
    if (deo.redshift)
        HIP_TRY(hipMemcpyAsync(deo.redshift, heo->redshift, 8 * K * N, hipMemcpyHostToDevice, st));
    if (emit_body(c, st, a)) return -1;
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
    if (deo.count) HIP_TRY(hipMemcpy(heo->count, deo.count, 4 * N, hipMemcpyDeviceToHost));
    if (deo.radius)
        HIP_TRY(hipMemcpy(heo->radius, deo.radius, 8 * K * N, hipMemcpyDeviceToHost));
    if (deo.redshift)
        HIP_TRY(hipMemcpy(heo->redshift, deo.redshift, 8 * K * N, hipMemcpyDeviceToHost));
    if (deo.intensity)
        HIP_TRY(hipMemcpy(heo->intensity, deo.intensity, 8 * N, hipMemcpyDeviceToHost));
    return 0;
}

int bhrt_kerr_emit_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         int flags, const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag,
                         const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (emit_frame_check(bh, dk, cfg, cam, W, H, NULL, flags, out, ep, eo, &k, &nrows)) return -1;
    emit_call a = {bh,   dk, cfg,   cam, W,    H,  nrows, NULL,
                   NULL, 0,  flags, out, diag, ep, eo,    &k};
    return emit_host(&a, NULL, (long)nrows * W);
}

int bhrt_kerr_emit_rays(const Ray* rays, int n, const BlackHoleParams* bh,
                        const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                        const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag,
                        const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo) {
    bhrt_kerr_k k;
    if (emit_rays_check(rays, n, bh, dk, cfg, flags, out, ep, eo, &k)) return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    emit_call a = {bh, dk, cfg, NULL, 0, 0, 0, NULL, NULL, n, flags, out, diag, ep, eo, &k};
    return emit_host(&a, rays, n);
}

int bhrt_kerr_disk_redshift(const BlackHoleParams* bh, double radius, double E, double lz,
                            double* g) {
    if (!bh || !g) {
        bhrt_set_err("kerr_emit: NULL argument");
        return -1;
    }
    const SimulationConfig cfg = {.time_step = 1.0};
    bhrt_kerr_k k;
    if (bhrt_kerr_scene(bh, NULL, &cfg, &k)) return -1;
    *g = bhrt_kerr_emit_g(radius, bh->spin * bh->mass, k.a2, k.M, E, lz);
    return 0;
}
