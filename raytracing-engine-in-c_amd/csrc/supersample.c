/*
 * supersample.c -- supersampled camera frames: every pixel is trace_pixel's sample average
 * (raytracer.c:1044-1167), at frame rate.
 *
 * A frame of n pixels and S samples is three steps on the caller's stream:
 *   k_ss_rays     the directions of the n * S sample rays, sample-major (ray s * n + p is shard
 *                 pixel p at sample s), from the camera path's own camera_dir -- S small
 *                 launches, each with its sample's offset in the argument block's camera;
 *   the trace     ONE launch of n * S rays with a shared origin and packed directions -- the
 *                 path trace_rays_batch takes for rays of one origin (bhrt_api.c
 *                 bhrt_rays_on_device) -- writing each sample's class and colour;
 *   k_ss_resolve  per pixel, the S colours added in sample order from 0.0 and divided by S, the
 *                 display conversions, and sample 0's class.
 * The sample scratch (24 B of directions, 24 B of colour, 4 B of class per sample ray; 16 B of
 * hit point more where BHRT_FUSE_COLOUR=0 takes the separate colour pass) lies behind the
 * launch's own 176 B per ray in the SAME per-stream allocation (context.c bhrt_stream_scratch),
 * so frames on two streams never share it and it stays valid until the stream's resolve has run.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the two launchers named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <string.h>

#include "bhrt_host.h"

int bhrt_sample_offsets(const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                        double* offset_x, double* offset_y, int capacity) {
    int samples = ss ? ss->samples_per_pixel : 1; /* raytracer.c:1066-1093 */
    if (as && as->enable_adaptive) {              /* (edge_factor fixed at 1.0) */
        samples = as->min_samples;
        samples += (int)((as->max_samples - as->min_samples) * 1.0);
        if (samples > as->max_samples) samples = as->max_samples;
    }
    if (samples < 1 || samples > BHRT_SS_MAX_SAMPLES) {
        bhrt_set_err("supersampling: %d samples per pixel (1..%d)", samples, BHRT_SS_MAX_SAMPLES);
        return -1;
    }
    const int jittered = ss && ss->samples_per_pixel > 1;
    if (jittered && ss->jitter_method == JITTER_RANDOM) {
        bhrt_set_err("supersampling: JITTER_RANDOM draws rand() per pixel and is not "
                     "reproducible; use the regular grid or Halton");
        return -1;
    }
    if (!offset_x || !offset_y || capacity < samples) {
        bhrt_set_err("supersampling: %d sample offsets need two arrays of that capacity (%d)",
                     samples, capacity);
        return -1;
    }
    for (int s = 0; s < samples; s++) {
        offset_x[s] = offset_y[s] = 0.5;
        if (jittered)
            bhrt_jitter(s, ss->samples_per_pixel, ss->jitter_method, ss->jitter_strength,
                        &offset_x[s], &offset_y[s]);
    }
    return samples;
}

/* the fields a supersampled frame can produce, as bits in bhrt_frame_soa's order: result (0),
 * rgb_r/g/b (10..12), rgba32f (13), rgba8 (14) */
#define SS_FIELDS 0x7c01u

typedef bhrt_ss_plan ss_plan;

/* the frame's arguments: 0 and the plan, or -1 (no HIP call) */
int bhrt_ss_check(const BlackHoleParams* bh, const SimulationConfig* cfg, const bhrt_camera* cam,
                  int W, int H, const bhrt_rows* rows, const SupersamplingParams* ss,
                  const AdaptiveSamplingParams* as, const bhrt_frame_soa* out, ss_plan* k) {
    if (!bh || !cfg || !cam || !out || W <= 0 || H <= 0) {
        bhrt_set_err("supersampled frame: invalid argument");
        return -1;
    }
    const int nrows = bhrt_shard_rows(H, rows);
    if (nrows < 0 || (long)nrows * W > INT_MAX) {
        bhrt_set_err("invalid row sharding or frame too large (%d x %d)", W, H);
        return -1;
    }
    if (cam->use_offset) {
        bhrt_set_err("supersampled frame: camera->use_offset must be 0 (the samples set the "
                     "sub-pixel offsets)");
        return -1;
    }
    void* const* f = (void* const*)out;
    for (int i = 0; i < BHRT_NFIELDS; i++)
        if (f[i] && !(SS_FIELDS >> i & 1u)) {
            bhrt_set_err("supersampled frame: only result, rgb_r/g/b, rgba32f and rgba8 are "
                         "produced (field %d is not NULL)", i);
            return -1;
        }
    if ((out->rgb_r || out->rgb_g || out->rgb_b) && !(out->rgb_r && out->rgb_g && out->rgb_b)) {
        bhrt_set_err("rgb output needs all of rgb_r/g/b");
        return -1;
    }
    const int samples = bhrt_sample_offsets(ss, as, k->off_x, k->off_y, BHRT_SS_MAX_SAMPLES);
    if (samples < 0) return -1;
    if ((long long)nrows * W * samples > INT_MAX) {
        bhrt_set_err("supersampled frame: %d x %d pixels of %d samples are more than %d rays", W,
                     nrows, samples, INT_MAX);
        return -1;
    }
    k->n = nrows * W;
    k->samples = samples;
    return 0;
}

/* the frame on `st` (not NULL) of context c */
static int ss_frame(devctx_t* c, hipStream_t st, const BlackHoleParams* bh,
                    const AccretionDiskParams* dk, const SimulationConfig* cfg,
                    const bhrt_camera* cam, int W, int H, const bhrt_rows* rows,
                    IntegrationMethod method, int flags, const ss_plan* k,
                    const bhrt_frame_soa* out) {
    const int n = k->n;
    if (n == 0) return 0;
    const size_t N = (size_t)n * (size_t)k->samples;
    const int fused = bhrt_colour_fused((int)method, dk != NULL, bh->spin != 0.0);
    /* the trace launch's own scratch first (what bhrt_rays_on_device asks for), then ours */
    const size_t launch_bytes = align256((size_t)BHRT_SCRATCH_FIELDS * sizeof(double) * N);
    const size_t plane8 = align256(8 * N), plane4 = align256(4 * N);
    const size_t bytes = launch_bytes + align256(24 * N) + 3 * plane8 + plane4 +
                         (fused ? 0 : 2 * plane8);
    char* p = (char*)bhrt_stream_scratch(c, st, bytes);
    if (!p) return -1;
    p += launch_bytes;
    bhrt_frame_soa smp; /* the sample planes the trace writes */
    memset(&smp, 0, sizeof smp);
    double* dirs = (double*)p;
    p += align256(24 * N);
    smp.rgb_r = (double*)p;
    smp.rgb_g = (double*)(p + plane8);
    smp.rgb_b = (double*)(p + 2 * plane8);
    p += 3 * plane8;
    smp.result = (int32_t*)p;
    p += plane4;
    if (!fused) { /* the separate colour pass reads the class and the hit point */
        smp.hit_x = (double*)p;
        smp.hit_y = (double*)(p + plane8);
    }
    bhrt_kparams kp;
    if (bhrt_fill_scene(&kp, bh, dk, cfg, method, flags)) return -1;
    bhrt_fill_camera(&kp, cam, W, H);
    if (rows && rows->num_shards > 1) { /* (as bhrt_frame_on_device sets a shard up) */
        kp.cam.rows = *rows;
        kp.cam.inv_block = 1.0 / (double)rows->row_block;
    }
    bhrt_ss_rays_k rk;
    memset(&rk, 0, sizeof rk);
    rk.cam = kp.cam;
    rk.n = n;
    rk.dirs = dirs;
    int e = 0;
    for (int s = 0; s < k->samples && e == 0; s++) { /* sample plane s: the frame at offset s */
        rk.cam.off_x = k->off_x[s];
        rk.cam.off_y = k->off_y[s];
        rk.sample = s;
        e = bhrt_launch_ss_rays(&rk, st);
    }
    if (e != 0) {
        bhrt_set_err("sample ray kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    if (bhrt_rays_on_device(NULL, dirs, (int)N, bh, dk, cfg, method, flags, &smp, st,
                            &cam->position))
        return -1;
    bhrt_ss_resolve_k r;
    memset(&r, 0, sizeof r);
    r.n = n;
    r.samples = k->samples;
    r.result = smp.result;
    r.r = smp.rgb_r;
    r.g = smp.rgb_g;
    r.b = smp.rgb_b;
    r.out = *out;
    e = bhrt_launch_ss_resolve(&r, st);
    if (e != 0) {
        bhrt_set_err("sample resolve kernel launch failed: %s",
                     hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

typedef struct { /* ss_frame's arguments, for its run under the stream rule */
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam;
    int W, H;
    const bhrt_rows* rows;
    IntegrationMethod method;
    int flags;
    const ss_plan* k;
    const bhrt_frame_soa* out;
} ss_call;

static int ss_body(devctx_t* c, hipStream_t st, const void* arg) {
    const ss_call* a = (const ss_call*)arg;
    return ss_frame(c, st, a->bh, a->dk, a->cfg, a->cam, a->W, a->H, a->rows, a->method, a->flags,
                    a->k, a->out);
}

int bhrt_render_frame_ss_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                                const bhrt_rows* rows, IntegrationMethod method, int flags,
                                const SupersamplingParams* ss, const AdaptiveSamplingParams* as,
                                const bhrt_frame_soa* out, void* stream) {
    ss_plan k;
    if (bhrt_ss_check(bh, cfg, cam, W, H, rows, ss, as, out, &k)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    /* NULL stream: the kernels run on libbhrt's own stream, after the caller's default-stream
     * work and before what it queues next */
    const ss_call a = {bh, dk, cfg, cam, W, H, rows, method, flags, &k, out};
    return bhrt_on_stream(c, (hipStream_t)stream, ss_body, &a);
}

int bhrt_render_frame_ss(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         IntegrationMethod method, int flags, const SupersamplingParams* ss,
                         const AdaptiveSamplingParams* as, const bhrt_frame_soa* out) {
    ss_plan k;
    if (bhrt_ss_check(bh, cfg, cam, W, H, NULL, ss, as, out, &k)) return -1;
    const int n = k.n;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    /* device outputs for the caller's fields (ss_check: all of them are fields a frame
     * produces), from the context's cached buffer */
    const size_t bytes = bhrt_soa_bytes(out, n);
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes ? bytes : 256, 0)) return -1;
    char* p = (char*)c->d_ss;
    bhrt_frame_soa dev;
    bhrt_soa_carve(&p, out, n, &dev);
    if (ss_frame(c, c->stream, bh, dk, cfg, cam, W, H, NULL, method, flags, &k, &dev)) return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* plain synchronous copies: caller memory is never page-locked */
    void* const* host = (void* const*)out;
    for (int i = 0; i < BHRT_NFIELDS; i++)
        if (host[i])
            HIP_TRY(hipMemcpy(host[i], ((void**)&dev)[i], k_fsize[i] * (size_t)n,
                              hipMemcpyDeviceToHost));
    return 0;
}
