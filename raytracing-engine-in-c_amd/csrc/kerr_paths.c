/*
 * kerr_paths.c -- physical photon paths: the recorded polylines of n rays traced as true null
 * geodesics of Kerr, in one launch (the rule: include/bhrt_api.h "Physical photon paths"; the
 * kernel: kerr.hip k_kerr_paths).
 *
 * The device form is its argument checks -- the path arguments and the hit arguments, every
 * refusal decided before any HIP call -- and one launch of k_kerr_paths on the caller's stream,
 * timed and counted like a trace launch: it takes a control block of the context's ring through
 * bhrt_ctx_launch_fn (the block's first word is the kernel's claim counter, zero at launch like the
 * rest), so it needs no scratch, no memset and no host wait. Where the caller asks for the rays'
 * hit records, bhrt_kerr_rays_device's own launch of the same rays follows it on the same stream
 * (kerr.c bhrt_kerr_rays_on_device). The host form uploads the rays, runs the same launches into
 * the context's cached device buffer and copies back what was stored (host_frames.c
 * bhrt_rows_back, the readback bhrt_trace_paths uses).
 *
 * A file of its own (the Makefile's HOST_FEATURE), not part of kerr.c: a program that links
 * kerr.c needs a stub of bhrt_launch_kerr alone, and the files of HOST_CORE none of either
 * (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

/* every argument: 0 and the scene's constants, or -1 with the error set; no HIP call, the current
 * device's query aside (BHRT_FLAG_SKY with hits) */
static int kpaths_check(const Ray* rays, int n, const BlackHoleParams* bh,
                        const AccretionDiskParams* dk, const SimulationConfig* cfg,
                        int max_positions, int every, int flags, const bhrt_paths* paths,
                        const bhrt_frame_soa* hits, const bhrt_kerr_diag* diag, bhrt_kerr_k* k) {
    if (bhrt_kerr_scene(bh, dk, cfg, k)) return -1;
    if (n <= 0) {
        bhrt_set_err("kerr paths: n = %d rays (at least 1)", n);
        return -1;
    }
    if (!rays) {
        bhrt_set_err("kerr paths: rays must not be NULL");
        return -1;
    }
    if (max_positions < 1 || max_positions > BHRT_PATHS_MAX_POSITIONS) {
        bhrt_set_err("kerr paths: max_positions = %d (1..%d)", max_positions,
                     BHRT_PATHS_MAX_POSITIONS);
        return -1;
    }
    if (every < 1) {
        bhrt_set_err("kerr paths: every = %d (at least 1)", every);
        return -1;
    }
    if (!paths || !(paths->xyz || paths->xyz32 || paths->count)) {
        bhrt_set_err("kerr paths: none of xyz, xyz32 and count is asked for");
        return -1;
    }
    if ((long)n * max_positions > INT_MAX) {
        bhrt_set_err("kerr paths: %d rays of %d positions are more than %d points", n,
                     max_positions, INT_MAX);
        return -1;
    }
    if (diag && !hits) {
        bhrt_set_err("kerr paths: the diagnostics come with the hit records (hits is NULL)");
        return -1;
    }
    return hits ? bhrt_kerr_out_bad(hits, flags) : 0;
}

static int kpaths_fn(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0, void* ev1) {
    return bhrt_launch_kerr_paths(kp, (const bhrt_kerr_paths_k*)arg, stream, ev0, ev1);
}

typedef struct { /* one checked call, for its run under the stream rule; device pointers */
    const Ray* d_rays;
    int n;
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    int max_positions, every, flags;
    const bhrt_paths* paths;
    const bhrt_frame_soa* hits;
    const bhrt_kerr_diag* diag;
    const bhrt_kerr_k* k;
} kpaths_call;

/* the launches on `st` of context c */
static int kpaths_body(devctx_t* c, hipStream_t st, const void* arg) {
    const kpaths_call* a = (const kpaths_call*)arg;
    bhrt_kparams kp;
    memset(&kp, 0, sizeof kp);
    kp.src = BHRT_SRC_RAYS;
    kp.rays = a->d_rays;
    kp.n = a->n;
    bhrt_kerr_paths_k pk;
    memset(&pk, 0, sizeof pk);
    pk.k = *a->k;
    pk.max_positions = a->max_positions;
    pk.every = a->every;
    pk.out = *a->paths;
    if (bhrt_ctx_launch_fn(c, &kp, st, kpaths_fn, &pk)) return -1;
    /* The hit records are k_kerr's own, from its own launch behind the path launch: "what
     * bhrt_kerr_rays_device writes", bit for bit, colour and sky map included. The two kernels
     * call one step and one set of tests (kerr.hip rk4_step, rk4_tests), each inlined into its own
     * schedule, and the contract between a path's last point and its hit_* stays a tolerance, not
     * every bit. bhrt_stats counts the two launches. */
    if (a->hits && bhrt_kerr_rays_on_device(c, st, a->d_rays, a->n, a->bh, a->dk, a->cfg, a->flags,
                                            a->hits, a->diag, a->k))
        return -1;
    return 0;
}

int bhrt_kerr_paths_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           int max_positions, int every, int flags, const bhrt_paths* paths,
                           const bhrt_frame_soa* hits, const bhrt_kerr_diag* diag, void* stream) {
    bhrt_kerr_k k;
    if (kpaths_check(d_rays, n, bh, dk, cfg, max_positions, every, flags, paths, hits, diag, &k))
        return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    /* NULL stream: the kernels run on libbhrt's own stream, after the caller's default-stream
     * work and before what it queues next */
    const kpaths_call a = {d_rays, n, bh, dk, cfg, max_positions, every, flags, paths, hits, diag,
                           &k};
    return bhrt_on_stream(c, (hipStream_t)stream, kpaths_body, &a);
}

int bhrt_kerr_paths(const Ray* rays, int n, const BlackHoleParams* bh,
                    const AccretionDiskParams* dk, const SimulationConfig* cfg, int max_positions,
                    int every, int flags, const bhrt_paths* paths, const bhrt_frame_soa* hits,
                    const bhrt_kerr_diag* diag) {
    bhrt_kerr_k k;
    if (kpaths_check(rays, n, bh, dk, cfg, max_positions, every, flags, paths, hits, diag, &k))
        return -1;
    for (long i = 0; i < n; i++)
        if (bhrt_kerr_observer(&k, &rays[i].origin, i)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    hipStream_t st = c->stream;
    const size_t P = (size_t)max_positions, N = (size_t)n;
    /* the context's cached buffer: rays, the counts (always: the readback goes by them), the
     * point arrays asked for, the hit fields and the diagnostics asked for */
    size_t bytes = align256(N * sizeof(Ray)) + align256(N * sizeof(int32_t));
    if (paths->xyz) bytes += align256(N * P * sizeof(Vector3D));
    if (paths->xyz32) bytes += align256(N * P * 3 * sizeof(float));
    /* (kerr.c's staging pieces for the hit records; the diagnostics are their two planes) */
    bhrt_kerr_diag ddiag = {NULL, NULL};
    const bhrt_kerr_plane pl[] = {{diag ? diag->h_residual : NULL, &ddiag.h_residual, 8 * N, 0},
                                  {diag ? diag->lz_drift : NULL, &ddiag.lz_drift, 8 * N, 0}};
    if (hits) bytes += bhrt_kerr_stage_bytes(hits, n, pl, 2);
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes, 0)) return -1;
    char* p = (char*)c->d_ss;
    Ray* d_rays = (Ray*)p;
    p += align256(N * sizeof(Ray));
    bhrt_paths dev;
    memset(&dev, 0, sizeof dev);
    dev.count = (int32_t*)p;
    p += align256(N * sizeof(int32_t));
    if (paths->xyz) {
        dev.xyz = (Vector3D*)p;
        p += align256(N * P * sizeof(Vector3D));
    }
    if (paths->xyz32) {
        dev.xyz32 = (float*)p;
        p += align256(N * P * 3 * sizeof(float));
    }
    bhrt_frame_soa dhits;
    HIP_TRY(hipMemcpyAsync(d_rays, rays, N * sizeof(Ray), hipMemcpyHostToDevice, st));
    if (hits && bhrt_kerr_stage_carve(&p, st, hits, n, &dhits, pl, 2)) return -1;
    const kpaths_call a = {d_rays, n, bh, dk, cfg, max_positions, every, flags, &dev,
                           hits ? &dhits : NULL, diag ? &ddiag : NULL, &k};
    if (kpaths_body(c, st, &a)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    /* plain synchronous copies: caller memory is never page-locked */
    int32_t* count = paths->count;
    int32_t* own_count = NULL;
    if (!count) {
        count = own_count = (int32_t*)malloc(N * sizeof(int32_t));
        if (!count) {
            bhrt_set_err("kerr paths: no memory for %d counts", n);
            return -1;
        }
    }
    int rc = 0;
    if (hipMemcpy(count, dev.count, N * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
        bhrt_set_err("kerr paths: readback failed: %s", hipGetErrorString(hipGetLastError()));
        rc = -1;
    }
    if (rc == 0 && paths->xyz)
        rc = bhrt_rows_back(paths->xyz, dev.xyz, count, n, P, sizeof(Vector3D));
    if (rc == 0 && paths->xyz32)
        rc = bhrt_rows_back(paths->xyz32, dev.xyz32, count, n, P, 3 * sizeof(float));
    free(own_count);
    if (rc) return -1;
    if (hits && bhrt_kerr_stage_back(hits, n, &dhits, pl, 2)) return -1;
    return 0;
}
