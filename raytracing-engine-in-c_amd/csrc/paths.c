/*
 * paths.c -- batched photon paths: the recorded polylines of n rays in one launch
 * (bhrt_api.h bhrt_trace_paths_device / bhrt_trace_paths; paths.hip k_paths).
 *
 * The device form is one launch of k_paths on the caller's stream, timed and counted like a
 * trace launch: it takes a control block of the context's ring through bhrt_ctx_launch_fn (the
 * block's first word is the kernel's claim counter, zero at launch like the rest), so it needs no
 * scratch of its own. Where the caller asks for the rays' hit records, a trace launch of the same
 * rays follows it on the same stream (paths_launch). The host form uploads the rays, runs the
 * same launches into the context's cached device buffer and copies back what was stored.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the launcher named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

/* the hit fields a path launch produces, as bits in bhrt_frame_soa's order: result, steps,
 * hit_x/y/z, distance, time_dilation, sky_x/y/z (0..9) */
#define HIT_FIELDS 0x3ffu

/* the arguments that need no device: 0, or -1 with the error set */
static int paths_check(const Ray* rays, int n, const BlackHoleParams* bh,
                       const SimulationConfig* cfg, int max_positions, int every,
                       const bhrt_paths* paths, const bhrt_frame_soa* hits) {
    if (n <= 0) {
        bhrt_set_err("paths: n = %d rays (at least 1)", n);
        return -1;
    }
    if (!rays || !bh || !cfg) {
        bhrt_set_err("paths: rays, blackhole and config must not be NULL");
        return -1;
    }
    if (max_positions < 1 || max_positions > BHRT_PATHS_MAX_POSITIONS) {
        bhrt_set_err("paths: max_positions = %d (1..%d)", max_positions, BHRT_PATHS_MAX_POSITIONS);
        return -1;
    }
    if (every < 1) {
        bhrt_set_err("paths: every = %d (at least 1)", every);
        return -1;
    }
    if (!paths || !(paths->xyz || paths->xyz32 || paths->count)) {
        bhrt_set_err("paths: none of xyz, xyz32 and count is asked for");
        return -1;
    }
    if ((long)n * max_positions > INT_MAX) {
        bhrt_set_err("paths: %d rays of %d positions are more than %d points", n, max_positions,
                     INT_MAX);
        return -1;
    }
    if (hits) {
        void* const* f = (void* const*)hits;
        for (int i = 0; i < BHRT_NFIELDS; i++)
            if (f[i] && !(HIT_FIELDS >> i & 1u)) {
                bhrt_set_err("paths: the hits carry no colour or display field (field %d is not "
                             "NULL)", i);
                return -1;
            }
    }
    return 0;
}

/* the store form: BHRT_PATHS_STORE=direct|staged, else the build's default */
static int paths_staged(void) {
    const char* e = getenv("BHRT_PATHS_STORE");
    if (e && strcmp(e, "direct") == 0) return 0;
    if (e && strcmp(e, "staged") == 0) return 1;
    return BHRT_PATHS_STAGED;
}

static int paths_fn(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0, void* ev1) {
    return bhrt_launch_paths(kp, (const bhrt_paths_k*)arg, stream, ev0, ev1);
}

/* the launch on `st` (not NULL) of context c; all pointers are device pointers */
static int paths_launch(devctx_t* c, hipStream_t st, const Ray* d_rays, int n,
                        const BlackHoleParams* bh, const AccretionDiskParams* dk,
                        const SimulationConfig* cfg,
                        IntegrationMethod method, int max_positions, int every,
                        const bhrt_paths* paths, const bhrt_frame_soa* hits) {
    bhrt_kparams kp;
    if (bhrt_check_scene(bh, cfg) || bhrt_fill_scene(&kp, bh, dk, cfg, method, 0)) return -1;
    kp.src = BHRT_SRC_RAYS;
    kp.rays = d_rays;
    kp.n = n;
    bhrt_paths_k pk;
    memset(&pk, 0, sizeof pk);
    pk.max_positions = max_positions;
    pk.every = every;
    pk.staged = paths_staged();
    pk.out = *paths;
    if (bhrt_ctx_launch_fn(c, &kp, st, paths_fn, &pk)) return -1;
    /* The hit records are the trace kernel's own, from its own launch behind the path launch:
     * "what bhrt_trace_rays_device writes", bit for bit. k_paths integrates with the single-ray
     * kernel's instantiation, so that its points are that kernel's bits; the trace kernel's
     * multi-iteration trips round a long ray's last bits differently (the end point of 17 of
     * 1000 C2 rays by up to 1.5e-15 relative, profiles/paths/hits_bits.txt), and one
     * integration cannot carry both. bhrt_stats counts the two launches. */
    if (hits && bhrt_rays_on_device(d_rays, NULL, n, bh, dk, cfg, method, 0, hits, st, NULL))
        return -1;
    return 0;
}

typedef struct { /* paths_launch's arguments, for its run under the stream rule */
    const Ray* d_rays;
    int n;
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    IntegrationMethod method;
    int max_positions, every;
    const bhrt_paths* paths;
    const bhrt_frame_soa* hits;
} paths_call;

static int paths_body(devctx_t* c, hipStream_t st, const void* arg) {
    const paths_call* a = (const paths_call*)arg;
    return paths_launch(c, st, a->d_rays, a->n, a->bh, a->dk, a->cfg, a->method, a->max_positions,
                        a->every, a->paths, a->hits);
}

int bhrt_trace_paths_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                            const AccretionDiskParams* dk, const SimulationConfig* cfg,
                            IntegrationMethod method, int max_positions, int every,
                            const bhrt_paths* paths, const bhrt_frame_soa* hits, void* stream) {
    if (paths_check(d_rays, n, bh, cfg, max_positions, every, paths, hits)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    /* NULL stream: the kernel runs on libbhrt's own stream, after the caller's default-stream
     * work and before what it queues next */
    const paths_call a = {d_rays, n, bh, dk, cfg, method, max_positions, every, paths, hits};
    return bhrt_on_stream(c, (hipStream_t)stream, paths_body, &a);
}

int bhrt_trace_paths(const Ray* rays, int n, const BlackHoleParams* bh,
                     const AccretionDiskParams* dk, const SimulationConfig* cfg,
                     IntegrationMethod method, int max_positions, int every,
                     const bhrt_paths* paths, const bhrt_frame_soa* hits) {
    if (paths_check(rays, n, bh, cfg, max_positions, every, paths, hits)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    hipStream_t st = c->stream;
    const size_t P = (size_t)max_positions, N = (size_t)n;
    /* the context's cached buffer: rays, the counts (always: the readback goes by them), the
     * point arrays asked for, the hit fields asked for */
    void* const* hhost = (void* const*)hits;
    size_t bytes = align256(N * sizeof(Ray)) + align256(N * sizeof(int32_t));
    if (paths->xyz) bytes += align256(N * P * sizeof(Vector3D));
    if (paths->xyz32) bytes += align256(N * P * 3 * sizeof(float));
    if (hits) bytes += bhrt_soa_bytes(hits, n);
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes ? bytes : 256, 0)) return -1;
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
    bhrt_frame_soa dhits; /* (paths_check: only fields a path launch produces) */
    if (hits) bhrt_soa_carve(&p, hits, n, &dhits);
    HIP_TRY(hipMemcpyAsync(d_rays, rays, N * sizeof(Ray), hipMemcpyHostToDevice, st));
    if (paths_launch(c, st, d_rays, n, bh, dk, cfg, method, max_positions, every, &dev,
                     hits ? &dhits : NULL))
        return -1;
    HIP_TRY(hipStreamSynchronize(st));
    /* plain synchronous copies: caller memory is never page-locked */
    int32_t* count = paths->count;
    int32_t* own_count = NULL;
    if (!count && (paths->xyz || paths->xyz32)) {
        count = own_count = (int32_t*)malloc(N * sizeof(int32_t));
        if (!count) {
            bhrt_set_err("paths: no memory for %d counts", n);
            return -1;
        }
    }
    int rc = 0;
    if (hipMemcpy(count, dev.count, N * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
        bhrt_set_err("paths: readback failed: %s", hipGetErrorString(hipGetLastError()));
        rc = -1;
    }
    if (rc == 0 && paths->xyz)
        rc = bhrt_rows_back(paths->xyz, dev.xyz, count, n, P, sizeof(Vector3D));
    if (rc == 0 && paths->xyz32)
        rc = bhrt_rows_back(paths->xyz32, dev.xyz32, count, n, P, 3 * sizeof(float));
    free(own_count);
    if (rc) return -1;
    for (int i = 0; hits && i < BHRT_NFIELDS; i++)
        if (hhost[i])
            HIP_TRY(hipMemcpy(hhost[i], ((void**)&dhits)[i], k_fsize[i] * N,
                              hipMemcpyDeviceToHost));
    return 0;
}
