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
 * launch (iterations: attempts). The call struct's shared part, the filling of the launch's
 * arguments and the host forms' staging are kerr.c's (bhrt_kerr_call, bhrt_kerr_fill,
 * bhrt_kerr_host); this file adds the emission's parameters and its four output planes. radius
 * and redshift elements beyond a ray's count are not written, so their device planes start from
 * the caller's values.
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

/* a camera call's checks (kerr.c's and the emission's): 0 and the shard's rows */
static int emit_frame_check(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            const bhrt_rows* rows, int flags, const bhrt_frame_soa* out,
                            const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo,
                            bhrt_kerr_k* k, int* nrows) {
    if (bhrt_kerr_scene(bh, dk, cfg, k) || bhrt_kerr_out_bad(out, flags) ||
        bhrt_kerr_frame_check("kerr_emit", cam, W, H, rows, nrows) ||
        emit_bad(dk, cfg, flags, out, ep, eo, (long)*nrows * W))
        return -1;
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
    bhrt_kerr_call c;
    int* rejected; /* bhrt_kerr_rk45_diag's third plane or NULL */
    const bhrt_kerr_emit_params* ep;
    bhrt_kerr_emit_out eo; /* NULL fields: not asked for */
} emit_call;

static const bhrt_kerr_emit_out k_no_emit_out = {NULL, NULL, NULL, NULL};

/* the launch on `st` of context c (c NULL: the current device's, made here); device pointers */
static int emit_body(devctx_t* c, hipStream_t st, const void* arg) {
    const emit_call* a = (const emit_call*)arg;
    if (!c) c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    bhrt_kparams kp;
    bhrt_kerr_emit_k ek;
    memset(&ek, 0, sizeof ek);
    if (bhrt_kerr_fill(&a->c, &kp, &ek.rk.k)) return -1;
    ek.rk.tol = a->c.cfg->tolerance;
    ek.rk.rejected = a->rejected;
    ek.max_crossings = a->ep->max_crossings;
    ek.q = a->ep->emissivity_index;
    ek.gain = a->ep->gain;
    ek.spin_a = a->c.bh->spin * a->c.bh->mass;
    ek.out = a->eo;
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
    const emit_call a = {{bh, dk, cfg, cam, W, H, nrows, rows, NULL, 0, flags, out,
                          diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k},
                         diag ? diag->rejected : NULL, ep, eo ? *eo : k_no_emit_out};
    return bhrt_on_stream(NULL, (hipStream_t)stream, emit_body, &a);
}

int bhrt_kerr_emit_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                               const AccretionDiskParams* dk, const SimulationConfig* cfg,
                               int flags, const bhrt_frame_soa* out,
                               const bhrt_kerr_rk45_diag* diag, const bhrt_kerr_emit_params* ep,
                               const bhrt_kerr_emit_out* eo, void* stream) {
    bhrt_kerr_k k;
    if (emit_rays_check(d_rays, n, bh, dk, cfg, flags, out, ep, eo, &k)) return -1;
    const emit_call a = {{bh, dk, cfg, NULL, 0, 0, 0, NULL, d_rays, n, flags, out,
                          diag ? diag->h_residual : NULL,
                              diag ? diag->lz_drift : NULL, &k},
                         diag ? diag->rejected : NULL, ep, eo ? *eo : k_no_emit_out};
    return bhrt_on_stream(NULL, (hipStream_t)stream, emit_body, &a);
}

/* the host forms: `a` with the host out and host rays (or a camera), n rays in all; the
 * diagnostics and the emission's outputs are its seven planes. radius and redshift are written
 * below a ray's count alone, so they start from the caller's values. */
static int emit_host(emit_call* a, const bhrt_kerr_rk45_diag* diag, const bhrt_kerr_emit_out* eo,
                     const Ray* rays, long n) {
    const size_t N = (size_t)n, K = (size_t)a->ep->max_crossings;
    const bhrt_kerr_plane pl[] = {{diag ? diag->h_residual : NULL, &a->c.h_residual, 8 * N, 0},
                                  {diag ? diag->lz_drift : NULL, &a->c.lz_drift, 8 * N, 0},
                                  {diag ? diag->rejected : NULL, &a->rejected, 4 * N, 0},
                                  {eo ? eo->count : NULL, &a->eo.count, 4 * N, 0},
                                  {eo ? eo->radius : NULL, &a->eo.radius, 8 * K * N, 1},
                                  {eo ? eo->redshift : NULL, &a->eo.redshift, 8 * K * N, 1},
                                  {eo ? eo->intensity : NULL, &a->eo.intensity, 8 * N, 0}};
    return bhrt_kerr_host(&a->c, rays, n, pl, 7, emit_body, a);
}

int bhrt_kerr_emit_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         int flags, const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag,
                         const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo) {
    bhrt_kerr_k k;
    int nrows = 0;
    if (emit_frame_check(bh, dk, cfg, cam, W, H, NULL, flags, out, ep, eo, &k, &nrows)) return -1;
    emit_call a = {{bh, dk, cfg, cam, W, H, nrows, NULL, NULL, 0, flags, out, NULL, NULL, &k},
                   NULL, ep, k_no_emit_out};
    return emit_host(&a, diag, eo, NULL, (long)nrows * W);
}

int bhrt_kerr_emit_rays(const Ray* rays, int n, const BlackHoleParams* bh,
                        const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                        const bhrt_frame_soa* out, const bhrt_kerr_rk45_diag* diag,
                        const bhrt_kerr_emit_params* ep, const bhrt_kerr_emit_out* eo) {
    bhrt_kerr_k k;
    if (emit_rays_check(rays, n, bh, dk, cfg, flags, out, ep, eo, &k)) return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    emit_call a = {{bh, dk, cfg, NULL, 0, 0, 0, NULL, NULL, n, flags, out, NULL, NULL, &k},
                   NULL, ep, k_no_emit_out};
    return emit_host(&a, diag, eo, rays, n);
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
