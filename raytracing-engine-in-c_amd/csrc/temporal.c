/*
 * temporal.c -- temporal accumulation frames: one jittered sample per pixel per frame, blended
 * into a running image on the GPU (the rule: include/bhrt_api.h). The reference wrote the
 * arithmetic (accumulateFrame, detectEdges, finalizeAccumulatedFrame, renderer.cpp:1759-1877) and
 * never calls it; the order blend -> edges -> display is ours.
 *
 * One rendered step of an accumulator of n pixels, all on the caller's stream, no host wait:
 *   the trace     the plain camera frame's own launch (bhrt_api.c bhrt_frame_on_device) with the
 *                 step's offset in the camera, writing rgba32f into the accumulator's scratch
 *                 frame (16 B per pixel);
 *   k_ta_blend    steps 1 to 3 and 6: acc in place, the optional copy, the display bytes;
 *   k_ta_edges    step 5 on the updated acc, whole images only; left out where the threshold is
 *                 NaN (edge is 0 at creation and only this kernel writes it, so it stays 0).
 * The host-side state advances when the step has been queued. The accumulator owns one block:
 * acc [n][3], edge [n] and the scratch frame [n][4] floats. Steps of one accumulator share the
 * scratch frame, so the caller orders them (the header says so).
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the two launchers named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

struct bhrt_accum {
    int device, W, H, n;
    int sharded;          /* rows split the image: no edge factors */
    bhrt_rows rows;
    bhrt_accum_params par;
    int frame_count, jitter_index, reset_pending;
    int64_t frames_total;
    void* d_base;         /* the one allocation */
    float *d_acc, *d_edge, *d_frame;
    void* d_host;         /* bhrt_accum_frame: device outputs of the host form */
    size_t cap_host;
    hipStream_t last;     /* the stream of the last step (bhrt_accum_destroy waits for it) */
    int used;
};

static const bhrt_accum_params k_defaults = {BHRT_ACCUM_REFERENCE, 0.1f, 32, 0.1f, 0.2f};

float bhrt_accum_alpha(const bhrt_accum_params* params, int frame_count) {
    const bhrt_accum_params* p = params ? params : &k_defaults;
    if (p->schedule == BHRT_ACCUM_MEAN) return 1.0f / (float)(frame_count + 1);
    if (frame_count == 0) return 1.0f; /* renderer.cpp:1771-1782 */
    if (frame_count < 5) return 0.5f;
    return p->blend_factor;
}

int bhrt_accum_create(int W, int H, const bhrt_rows* rows, const bhrt_accum_params* params,
                      bhrt_accum** acc) {
    const bhrt_accum_params par = params ? *params : k_defaults;
    if (!acc || W < 1 || H < 1) {
        bhrt_set_err("accumulator: invalid argument (%d x %d)", W, H);
        return -1;
    }
    const int nrows = bhrt_shard_rows(H, rows);
    if (nrows < 0 || (long long)W * H > INT_MAX) {
        bhrt_set_err("accumulator: invalid row sharding or image too large (%d x %d)", W, H);
        return -1;
    }
    if (par.schedule != BHRT_ACCUM_REFERENCE && par.schedule != BHRT_ACCUM_MEAN) {
        bhrt_set_err("accumulator: unknown schedule %d", (int)par.schedule);
        return -1;
    }
    if (!(par.blend_factor >= 0.0f && par.blend_factor <= 1.0f)) { /* (false for NaN) */
        bhrt_set_err("accumulator: blend_factor %g is not in [0, 1]", (double)par.blend_factor);
        return -1;
    }
    if (par.max_frames < 1) {
        bhrt_set_err("accumulator: max_frames %d (>= 1)", (int)par.max_frames);
        return -1;
    }
    if (!(par.edge_decay >= 0.0f)) {
        bhrt_set_err("accumulator: edge_decay %g is negative or NaN", (double)par.edge_decay);
        return -1;
    }
    const int dev = bhrt_current_device();
    if (dev < 0) {
        bhrt_set_err("accumulator: no current device");
        return -1;
    }
    bhrt_accum* a = (bhrt_accum*)calloc(1, sizeof *a);
    if (!a) {
        bhrt_set_err("accumulator: out of memory");
        return -1;
    }
    a->device = dev;
    a->W = W;
    a->H = H;
    a->n = nrows * W;
    a->sharded = rows && rows->num_shards > 1;
    if (a->sharded) a->rows = *rows;
    else a->rows = (bhrt_rows){0, 0, 1};
    a->par = par;
    a->reset_pending = 1;
    const size_t n = (size_t)a->n;
    const size_t b_acc = align256(12 * n), b_edge = align256(4 * n), b_frame = align256(16 * n);
    const size_t bytes = b_acc + b_edge + b_frame + 256; /* (never empty: a shard without rows) */
    const hipError_t he = hipMalloc(&a->d_base, bytes);
    if (he != hipSuccess) {
        bhrt_set_err("accumulator: allocation of %zu bytes failed: %s", bytes,
                     hipGetErrorString(he));
        free(a);
        return -1;
    }
    a->d_acc = (float*)a->d_base;
    a->d_edge = (float*)((char*)a->d_base + b_acc);
    a->d_frame = (float*)((char*)a->d_base + b_acc + b_edge);
    /* acc = 0 and edge = 0, complete before any stream can read them */
    if (hipMemsetAsync(a->d_base, 0, b_acc + b_edge, (hipStream_t)0) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)0) != hipSuccess) {
        bhrt_set_err("accumulator: cannot zero the state arrays");
        (void)hipFree(a->d_base);
        free(a);
        return -1;
    }
    *acc = a;
    return 0;
}

void bhrt_accum_destroy(bhrt_accum* a) {
    if (!a) return;
    if (a->used) (void)hipStreamSynchronize(a->last);
    if (a->d_host) (void)hipFree(a->d_host);
    (void)hipFree(a->d_base);
    free(a);
}

int bhrt_accum_reset(bhrt_accum* a) {
    if (!a) {
        bhrt_set_err("accumulator: NULL handle");
        return -1;
    }
    a->reset_pending = 1;
    return 0;
}

/* the sample set of ss (NULL: the pixel centre alone): the count, or -1 with the error set */
static int ta_offsets(const SupersamplingParams* ss, double* ox, double* oy) {
    return bhrt_sample_offsets(ss, NULL, ox, oy, BHRT_SS_MAX_SAMPLES);
}

int bhrt_accum_info(const bhrt_accum* a, const SupersamplingParams* ss, bhrt_accum_state* s) {
    if (!a || !s) {
        bhrt_set_err("accumulator: NULL argument");
        return -1;
    }
    double ox[BHRT_SS_MAX_SAMPLES], oy[BHRT_SS_MAX_SAMPLES];
    const int cycle = ta_offsets(ss, ox, oy);
    if (cycle < 0) return -1;
    memset(s, 0, sizeof *s);
    s->frame_count = a->frame_count;
    s->jitter_index = a->jitter_index;
    s->reset_pending = a->reset_pending;
    s->cycle = cycle;
    s->next_alpha = bhrt_accum_alpha(&a->par, a->reset_pending ? 0 : a->frame_count);
    s->sharded = a->sharded;
    s->next_offset_x = ox[a->jitter_index % cycle];
    s->next_offset_y = oy[a->jitter_index % cycle];
    s->frames_total = a->frames_total;
    s->pixels = a->n;
    return 0;
}

int bhrt_accum_device_buffers(const bhrt_accum* a, const float** rgb, const float** edge) {
    if (!a) {
        bhrt_set_err("accumulator: NULL handle");
        return -1;
    }
    if (rgb) *rgb = a->d_acc;
    if (edge) *edge = a->d_edge;
    return 0;
}

typedef struct { /* one step, for its run under the stream rule */
    bhrt_accum* a;
    const float* frame; /* a caller's [n][3] frame, or NULL: render */
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam; /* the step's offset already in it */
    IntegrationMethod method;
    int flags;
    const bhrt_accum_out* out;
} ta_call;

static int ta_body(devctx_t* c, hipStream_t st, const void* arg) {
    const ta_call* k = (const ta_call*)arg;
    bhrt_accum* a = k->a;
    if (a->n == 0) return 0; /* (a shard without rows) */
    if (!k->frame) {
        bhrt_frame_soa soa;
        memset(&soa, 0, sizeof soa);
        soa.rgba32f = a->d_frame;
        if (bhrt_frame_on_device(k->bh, k->dk, k->cfg, k->cam, a->W, a->H,
                                 a->sharded ? &a->rows : NULL, k->method, k->flags, &soa, st, 1))
            return -1;
    }
    const int fc = a->reset_pending ? 0 : a->frame_count;
    bhrt_ta_blend_k b;
    memset(&b, 0, sizeof b);
    b.n = a->n;
    b.frame = k->frame ? k->frame : a->d_frame;
    b.stride = k->frame ? 3 : 4;
    b.zero = a->reset_pending;
    b.alpha = bhrt_accum_alpha(&a->par, fc);
    b.w = 1.0f - b.alpha;
    b.acc = a->d_acc;
    b.rgb = k->out ? k->out->rgb : NULL;
    b.rgba8 = k->out ? k->out->rgba8 : NULL;
    int e = bhrt_launch_ta_blend(&b, st);
    if (e != 0) {
        bhrt_set_err("accumulator blend kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    float* edge_out = k->out ? k->out->edge_factor : NULL;
    if (!a->sharded && a->par.edge_threshold == a->par.edge_threshold) {
        bhrt_ta_edges_k ek;
        memset(&ek, 0, sizeof ek);
        ek.n = a->n;
        ek.width = a->W;
        ek.height = a->H;
        ek.threshold = a->par.edge_threshold;
        ek.decay = a->par.edge_decay;
        ek.acc = a->d_acc;
        ek.edge = a->d_edge;
        ek.out = edge_out;
        e = bhrt_launch_ta_edges(&ek, st);
        if (e != 0) {
            bhrt_set_err("accumulator edge kernel launch failed: %s",
                         hipGetErrorString((hipError_t)e));
            return -1;
        }
    } else if (edge_out) { /* a NaN threshold: the zeros of creation */
        HIP_TRY(hipMemcpyAsync(edge_out, a->d_edge, 4 * (size_t)a->n, hipMemcpyDeviceToDevice, st));
    }
    (void)c;
    return 0;
}

/* what a step refuses before any HIP call but the current device's query; the rendered step's
 * offset and cycle in *ox, *oy, *cycle */
static int ta_check(const bhrt_accum* a, int render, const BlackHoleParams* bh,
                    const SimulationConfig* cfg, const bhrt_camera* cam,
                    const SupersamplingParams* ss, const void* frame, const bhrt_accum_out* out,
                    double* ox, double* oy, int* cycle) {
    if (!a) {
        bhrt_set_err("accumulator: NULL handle");
        return -1;
    }
    if (render ? (!bh || !cfg || !cam || !out) : !frame) {
        bhrt_set_err("accumulator: NULL argument");
        return -1;
    }
    if (render) {
        if (cam->use_offset) {
            bhrt_set_err("accumulator: camera->use_offset must be 0 (the accumulator sets the "
                         "sub-pixel offsets)");
            return -1;
        }
        double sx[BHRT_SS_MAX_SAMPLES], sy[BHRT_SS_MAX_SAMPLES];
        *cycle = ta_offsets(ss, sx, sy);
        if (*cycle < 0) return -1;
        *ox = sx[a->jitter_index % *cycle];
        *oy = sy[a->jitter_index % *cycle];
        if (bhrt_check_scene(bh, cfg)) return -1;
    }
    if (out && out->edge_factor && a->sharded) {
        bhrt_set_err("accumulator: edge_factor needs a whole image (this accumulator holds shard "
                     "%d of %d)", a->rows.shard, a->rows.num_shards);
        return -1;
    }
    const int dev = bhrt_current_device();
    if (dev != a->device) {
        bhrt_set_err("accumulator: made on device %d, the current device is %d", a->device, dev);
        return -1;
    }
    return 0;
}

/* the step has been queued on st: steps 1 and 4 of the host-side state */
static void ta_advance(bhrt_accum* a, int cycle, hipStream_t st) {
    if (a->reset_pending) {
        a->frame_count = 0;
        a->reset_pending = 0;
    }
    a->frame_count = a->frame_count + 1 < a->par.max_frames ? a->frame_count + 1 : a->par.max_frames;
    a->jitter_index = (a->jitter_index % cycle + 1) % cycle;
    a->frames_total++;
    a->last = st;
    a->used = 1;
}

/* a checked step on `stream` under the device API's stream rule */
static int ta_step(bhrt_accum* a, ta_call* k, int cycle, hipStream_t stream) {
    devctx_t* c = bhrt_ctx_get(a->device);
    if (!c) return -1;
    if (bhrt_on_stream(c, stream, ta_body, k)) return -1;
    ta_advance(a, cycle, stream ? stream : c->stream);
    return 0;
}

int bhrt_accum_frame_device(bhrt_accum* a, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam,
                            IntegrationMethod method, int flags, const SupersamplingParams* ss,
                            const bhrt_accum_out* out, void* stream) {
    double ox = 0.5, oy = 0.5;
    int cycle = 1;
    if (ta_check(a, 1, bh, cfg, cam, ss, NULL, out, &ox, &oy, &cycle)) return -1;
    bhrt_camera at = *cam;
    at.use_offset = 1;
    at.offset_x = ox;
    at.offset_y = oy;
    ta_call k = {a, NULL, bh, dk, cfg, &at, method, flags, out};
    return ta_step(a, &k, cycle, (hipStream_t)stream);
}

int bhrt_accum_blend_device(bhrt_accum* a, const float* device_rgb, const bhrt_accum_out* out,
                            void* stream) {
    double ox, oy;
    int cycle;
    if (ta_check(a, 0, NULL, NULL, NULL, NULL, device_rgb, out, &ox, &oy, &cycle)) return -1;
    ta_call k = {a, device_rgb, NULL, NULL, NULL, NULL, INTEGRATOR_RK4, 0, out};
    return ta_step(a, &k, BHRT_SS_MAX_SAMPLES, (hipStream_t)stream);
}

int bhrt_accum_frame(bhrt_accum* a, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                     const SimulationConfig* cfg, const bhrt_camera* cam, IntegrationMethod method,
                     int flags, const SupersamplingParams* ss, const bhrt_accum_out* out) {
    double ox = 0.5, oy = 0.5;
    int cycle = 1;
    if (ta_check(a, 1, bh, cfg, cam, ss, NULL, out, &ox, &oy, &cycle)) return -1;
    bhrt_camera at = *cam;
    at.use_offset = 1;
    at.offset_x = ox;
    at.offset_y = oy;
    devctx_t* c = bhrt_ctx_get(a->device);
    if (!c || bhrt_ctx_streams(c)) return -1;
    /* device outputs for the caller's arrays, kept with the accumulator */
    const size_t n = (size_t)a->n;
    const size_t b8 = align256(4 * n), b3 = align256(12 * n), b1 = align256(4 * n);
    if (bhrt_ensure(&a->d_host, &a->cap_host, b8 + b3 + b1 + 256, 0)) return -1;
    bhrt_accum_out dev = {NULL, NULL, NULL};
    if (out->rgba8) dev.rgba8 = (uint8_t*)a->d_host;
    if (out->rgb) dev.rgb = (float*)((char*)a->d_host + b8);
    if (out->edge_factor) dev.edge_factor = (float*)((char*)a->d_host + b8 + b3);
    ta_call k = {a, NULL, bh, dk, cfg, &at, method, flags, &dev};
    if (ta_body(c, c->stream, &k)) return -1;
    ta_advance(a, cycle, c->stream);
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* plain synchronous copies: caller memory is never page-locked */
    if (out->rgba8) HIP_TRY(hipMemcpy(out->rgba8, dev.rgba8, 4 * n, hipMemcpyDeviceToHost));
    if (out->rgb) HIP_TRY(hipMemcpy(out->rgb, dev.rgb, 12 * n, hipMemcpyDeviceToHost));
    if (out->edge_factor)
        HIP_TRY(hipMemcpy(out->edge_factor, dev.edge_factor, 4 * n, hipMemcpyDeviceToHost));
    return 0;
}
