/*
 * adaptive.c -- adaptive supersampled camera frames: every pixel gets min_samples samples, and
 * only the pixels the edge rule marks get max_samples (the rule: include/bhrt_api.h,
 * bhrt_render_frame_adaptive_device). The reference has the parameters and the stencil
 * (raytracer.c:1074-1093, renderer.cpp:1802-1853) but never joins them: its edge factor is 1.0.
 *
 * A shard of n owned pixels, B = min_samples, M = max_samples, on the caller's stream:
 *   base pass     k_ad_rays (B launches, the sample's offset in the argument block's camera) for
 *                 the ext pixels -- the shard's rows and its halo rows, the image rows next to
 *                 them that another shard owns -- then ONE shared-origin trace of next * B rays
 *                 (bhrt_rays_on_device, the supersampled frame's path) into the base planes;
 *   k_ad_edges    the base colour, the 4-neighbour stencil in the image, the decision, and the
 *                 edge pixels compacted into a list with each pixel's slot;
 *   hand-over     the edge count E read into pinned memory by one 8-byte copy, and a host wait
 *                 on the stream: the second launch's size exists only on the device, and the
 *                 trace kernel takes its ray count from the host;
 *   extra pass    k_ad_rays (M - B launches) over the edge list and ONE trace of E * (M - B)
 *                 rays, extra ray (s - B) * E + slot; left out where E == 0 or M == B;
 *   k_ad_resolve  the sequential sum over a pixel's base samples, continued over its extra
 *                 samples, divided by S(p); the outputs, the class and S(p).
 * Memory: the base planes, the list, the slots, the counter and the row tables lie in the
 * stream's SECOND block (context.c bhrt_stream_keep), which no request for the launch scratch
 * moves; the extra planes, sized once E is known, lie behind the second launch's own scratch in
 * the stream's first block (as supersample.c places its planes), which may be a new allocation
 * by then -- the first launch has completed when the host asks for it.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the three launchers named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <string.h>

#include "bhrt_host.h"

typedef struct { /* a checked frame */
    bhrt_ss_plan ss;    /* owned pixels, M and the M offsets */
    int base, max;      /* B, M */
    int sharded;        /* rows split the image */
    int ext_rows, halo_rows;
} ad_plan;

static int ad_owned(int y, const bhrt_rows* rows) {
    return (y / rows->row_block) % rows->num_shards == rows->shard;
}

/* The ext rows of a shard, ascending: image row y is one if the shard owns it or owns a row next
 * to it. Writes rows_out[e] = y and ext_of[y] = e or -1 where the arrays are given; returns the
 * number of ext rows and in *halo how many of them the shard does not own. */
static int ad_rows(int H, const bhrt_rows* rows, int* rows_out, int* ext_of, int* halo) {
    int e = 0, h = 0;
    for (int y = 0; y < H; y++) {
        const int own = ad_owned(y, rows);
        const int near = own || (y > 0 && ad_owned(y - 1, rows)) ||
                         (y + 1 < H && ad_owned(y + 1, rows));
        if (ext_of) ext_of[y] = near ? e : -1;
        if (!near) continue;
        if (rows_out) rows_out[e] = y;
        h += !own;
        e++;
    }
    *halo = h;
    return e;
}

/* the frame's arguments: 0 and the plan, or -1 (no HIP call) */
static int ad_check(const BlackHoleParams* bh, const SimulationConfig* cfg, const bhrt_camera* cam,
                    int W, int H, const bhrt_rows* rows, const SupersamplingParams* ss,
                    const AdaptiveSamplingParams* as, const bhrt_frame_soa* out, ad_plan* k) {
    if (!as || !as->enable_adaptive) {
        bhrt_set_err("adaptive frame: needs AdaptiveSamplingParams with enable_adaptive set");
        return -1;
    }
    if (as->min_samples < 1 || as->max_samples < as->min_samples ||
        as->max_samples > BHRT_SS_MAX_SAMPLES) {
        bhrt_set_err("adaptive frame: min_samples %d, max_samples %d (1 <= min <= max <= %d)",
                     as->min_samples, as->max_samples, BHRT_SS_MAX_SAMPLES);
        return -1;
    }
    /* everything the supersampled frame of M samples refuses; the plan's offsets are the first
     * M of bhrt_sample_offsets(ss, as) */
    if (bhrt_ss_check(bh, cfg, cam, W, H, rows, ss, as, out, &k->ss)) return -1;
    if ((long long)W * H > INT_MAX) { /* (rays are addressed by image pixel) */
        bhrt_set_err("adaptive frame: %d x %d pixels are more than %d", W, H, INT_MAX);
        return -1;
    }
    k->base = as->min_samples;
    k->max = as->max_samples;
    k->sharded = rows && rows->num_shards > 1;
    k->ext_rows = H;
    k->halo_rows = 0;
    if (k->sharded) k->ext_rows = ad_rows(H, rows, NULL, NULL, &k->halo_rows);
    if ((long long)k->ext_rows * W * k->base > INT_MAX) {
        bhrt_set_err("adaptive frame: the base pass of %d x %d pixels (halo rows included) and %d "
                     "samples is more than %d rays", W, k->ext_rows, k->base, INT_MAX);
        return -1;
    }
    return 0;
}

static void ad_info(bhrt_adaptive_info* info, const ad_plan* k, int W, long long edges) {
    if (!info) return;
    info->pixels = k->ss.n;
    info->edge_pixels = edges;
    info->halo_pixels = (int64_t)k->halo_rows * W;
    info->sample_rays = (info->pixels + info->halo_pixels) * k->base + edges * (k->max - k->base);
}

/* the sample planes a trace of N rays writes, carved from *p */
static void ad_planes(char** p, size_t N, int fused, int with_class, bhrt_frame_soa* smp) {
    const size_t plane8 = align256(8 * N);
    memset(smp, 0, sizeof *smp);
    smp->rgb_r = (double*)*p;
    smp->rgb_g = (double*)(*p + plane8);
    smp->rgb_b = (double*)(*p + 2 * plane8);
    *p += 3 * plane8;
    if (with_class || !fused) {
        smp->result = (int32_t*)*p;
        *p += align256(4 * N);
    }
    if (!fused) { /* the separate colour pass reads the class and the hit point */
        smp->hit_x = (double*)*p;
        smp->hit_y = (double*)(*p + plane8);
        *p += 2 * plane8;
    }
}

static size_t ad_planes_bytes(size_t N, int fused, int with_class) {
    return 3 * align256(8 * N) + (with_class || !fused ? align256(4 * N) : 0) +
           (fused ? 0 : 2 * align256(8 * N));
}

/* one pass's directions: a launch per sample, the sample's offset in the block's camera */
static int ad_dirs(bhrt_ad_rays_k* rk, const ad_plan* k, int s0, int s1, hipStream_t st) {
    for (int s = s0; s < s1; s++) {
        rk->cam.off_x = k->ss.off_x[s];
        rk->cam.off_y = k->ss.off_y[s];
        rk->first = (long)(s - s0) * rk->n;
        const int e = bhrt_launch_ad_rays(rk, st);
        if (e != 0) {
            bhrt_set_err("adaptive ray kernel launch failed: %s", hipGetErrorString((hipError_t)e));
            return -1;
        }
    }
    return 0;
}

/* the frame on `st` (not NULL) of context c */
static int ad_frame(devctx_t* c, hipStream_t st, const BlackHoleParams* bh,
                    const AccretionDiskParams* dk, const SimulationConfig* cfg,
                    const bhrt_camera* cam, int W, int H, const bhrt_rows* rows,
                    IntegrationMethod method, int flags, const ad_plan* k, double threshold,
                    const bhrt_frame_soa* out, int32_t* samples, bhrt_adaptive_info* info) {
    const int n = k->ss.n, B = k->base, M = k->max;
    if (n == 0) { /* (a shard without rows traces nothing) */
        if (info) memset(info, 0, sizeof *info);
        return 0;
    }
    const size_t next = (size_t)k->ext_rows * (size_t)W, Nb = next * (size_t)B;
    const int fused = bhrt_colour_fused((int)method, dk != NULL, bh->spin != 0.0);
    /* pinned: the count, then (a shard's) row tables */
    const size_t tab_bytes = k->sharded ? 4 * ((size_t)k->ext_rows + (size_t)H) : 0;
    if (bhrt_ensure(&c->h_ad, &c->cap_ad, 256 + tab_bytes, 1)) return -1;
    unsigned long long* h_count = (unsigned long long*)c->h_ad;
    /* the stream's second block: what must survive the second launch's allocation */
    const size_t bytes = align256(24 * Nb) + ad_planes_bytes(Nb, fused, 1) +
                         2 * align256(4 * (size_t)n) + 256 + align256(tab_bytes);
    char* p = (char*)bhrt_stream_keep(c, st, bytes);
    if (!p) return -1;
    double* dirs = (double*)p;
    p += align256(24 * Nb);
    bhrt_frame_soa smp;
    ad_planes(&p, Nb, fused, 1, &smp);
    int* d_slot = (int*)p;
    p += align256(4 * (size_t)n);
    int* d_list = (int*)p;
    p += align256(4 * (size_t)n);
    unsigned long long* d_count = (unsigned long long*)p;
    p += 256;
    const int *d_rows = NULL, *d_ext_of = NULL;
    if (k->sharded) {
        int* h_tab = (int*)((char*)c->h_ad + 256);
        int halo;
        ad_rows(H, rows, h_tab, h_tab + k->ext_rows, &halo);
        HIP_TRY(hipMemcpyAsync(p, h_tab, tab_bytes, hipMemcpyHostToDevice, st));
        d_rows = (const int*)p;
        d_ext_of = d_rows + k->ext_rows;
    }
    /* the whole image's camera: rays are addressed by image pixel */
    bhrt_kparams kp;
    if (bhrt_fill_scene(&kp, bh, dk, cfg, method, flags)) return -1;
    bhrt_fill_camera(&kp, cam, W, H);
    bhrt_ad_rays_k rk;
    memset(&rk, 0, sizeof rk);
    rk.cam = kp.cam;
    rk.n = (int)next;
    rk.rows = d_rows;
    rk.dirs = dirs;
    if (ad_dirs(&rk, k, 0, B, st)) return -1;
    if (bhrt_rays_on_device(NULL, dirs, (int)Nb, bh, dk, cfg, method, flags, &smp, st,
                            &cam->position))
        return -1;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof *d_count, st));
    bhrt_ad_edges_k ek;
    memset(&ek, 0, sizeof ek);
    ek.n = n;
    ek.width = W;
    ek.height = H;
    ek.inv_width = kp.cam.inv_width;
    ek.rows = kp.cam.rows;
    ek.inv_block = kp.cam.inv_block;
    if (k->sharded) {
        ek.rows = *rows;
        ek.inv_block = 1.0 / (double)rows->row_block;
    }
    ek.ext_of = d_ext_of;
    ek.next = (long)next;
    ek.base = B;
    ek.max = M;
    ek.threshold = threshold;
    ek.r = smp.rgb_r;
    ek.g = smp.rgb_g;
    ek.b = smp.rgb_b;
    ek.slot = d_slot;
    ek.list = d_list;
    ek.count = d_count;
    int e = bhrt_launch_ad_edges(&ek, st);
    if (e != 0) {
        bhrt_set_err("adaptive edge kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    /* the hand-over: the second launch's size, from the device to the host */
    *h_count = 0;
    HIP_TRY(hipMemcpyAsync(h_count, d_count, sizeof *h_count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long edges = *h_count;
    if (edges > (unsigned long long)n) {
        bhrt_set_err("adaptive frame: edge count %llu of %d pixels", edges, n);
        return -1;
    }
    const size_t E = (size_t)edges, Nx = E * (size_t)(M - B);
    if (Nx > (size_t)INT_MAX) {
        bhrt_set_err("adaptive frame: the extra pass of %zu pixels and %d samples is more than %d "
                     "rays", E, M - B, INT_MAX);
        return -1;
    }
    ad_info(info, k, W, (long long)edges);
    bhrt_frame_soa xtr;
    memset(&xtr, 0, sizeof xtr);
    if (Nx > 0) {
        /* the second launch's own scratch first (what bhrt_rays_on_device asks for), then ours */
        const size_t launch_bytes = align256((size_t)BHRT_SCRATCH_FIELDS * sizeof(double) * Nx);
        char* q = (char*)bhrt_stream_scratch(c, st, launch_bytes + align256(24 * Nx) +
                                                        ad_planes_bytes(Nx, fused, 0));
        if (!q) return -1;
        q += launch_bytes;
        double* xdirs = (double*)q;
        q += align256(24 * Nx);
        ad_planes(&q, Nx, fused, 0, &xtr);
        rk.n = (int)E;
        rk.rows = NULL;
        rk.pixels = d_list;
        rk.dirs = xdirs;
        if (ad_dirs(&rk, k, B, M, st)) return -1;
        if (bhrt_rays_on_device(NULL, xdirs, (int)Nx, bh, dk, cfg, method, flags, &xtr, st,
                                &cam->position))
            return -1;
    }
    bhrt_ad_resolve_k r;
    memset(&r, 0, sizeof r);
    r.n = n;
    r.width = W;
    r.height = H;
    r.rows = ek.rows;
    r.inv_width = ek.inv_width;
    r.inv_block = ek.inv_block;
    r.ext_of = d_ext_of;
    r.next = (long)next;
    r.nedge = (long)E;
    r.base = B;
    r.max = M;
    r.result = smp.result;
    r.r = smp.rgb_r;
    r.g = smp.rgb_g;
    r.b = smp.rgb_b;
    r.xr = xtr.rgb_r;
    r.xg = xtr.rgb_g;
    r.xb = xtr.rgb_b;
    r.slot = d_slot;
    r.out = *out;
    r.samples = samples;
    e = bhrt_launch_ad_resolve(&r, st);
    if (e != 0) {
        bhrt_set_err("adaptive resolve kernel launch failed: %s",
                     hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

typedef struct { /* ad_frame's arguments, for its run under the stream rule */
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam;
    int W, H;
    const bhrt_rows* rows;
    IntegrationMethod method;
    int flags;
    const ad_plan* k;
    double threshold;
    const bhrt_frame_soa* out;
    int32_t* samples;
    bhrt_adaptive_info* info;
} ad_call;

static int ad_body(devctx_t* c, hipStream_t st, const void* arg) {
    const ad_call* a = (const ad_call*)arg;
    return ad_frame(c, st, a->bh, a->dk, a->cfg, a->cam, a->W, a->H, a->rows, a->method, a->flags,
                    a->k, a->threshold, a->out, a->samples, a->info);
}

int bhrt_render_frame_adaptive_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                      const SimulationConfig* cfg, const bhrt_camera* cam, int W,
                                      int H, const bhrt_rows* rows, IntegrationMethod method,
                                      int flags, const SupersamplingParams* ss,
                                      const AdaptiveSamplingParams* as, const bhrt_frame_soa* out,
                                      int32_t* samples, bhrt_adaptive_info* info, void* stream) {
    ad_plan k;
    if (ad_check(bh, cfg, cam, W, H, rows, ss, as, out, &k)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    /* NULL stream: the kernels run on libbhrt's own stream, after the caller's default-stream
     * work and before what it queues next */
    const ad_call a = {bh, dk, cfg, cam, W, H, rows, method, flags, &k, as->edge_threshold, out,
                       samples, info};
    return bhrt_on_stream(c, (hipStream_t)stream, ad_body, &a);
}

int bhrt_render_frame_adaptive(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                               const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                               IntegrationMethod method, int flags, const SupersamplingParams* ss,
                               const AdaptiveSamplingParams* as, const bhrt_frame_soa* out,
                               int32_t* samples, bhrt_adaptive_info* info) {
    ad_plan k;
    if (ad_check(bh, cfg, cam, W, H, NULL, ss, as, out, &k)) return -1;
    const int n = k.ss.n;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c || bhrt_ctx_streams(c)) return -1;
    /* device outputs for the caller's fields and the sample counts, from the context's cached
     * buffer */
    const size_t bytes = bhrt_soa_bytes(out, n) + align256(4 * (size_t)n);
    if (bhrt_ensure(&c->d_ss, &c->cap_ss, bytes, 0)) return -1;
    char* p = (char*)c->d_ss;
    bhrt_frame_soa dev;
    bhrt_soa_carve(&p, out, n, &dev);
    int32_t* d_samples = samples ? (int32_t*)p : NULL;
    bhrt_adaptive_info got;
    if (ad_frame(c, c->stream, bh, dk, cfg, cam, W, H, NULL, method, flags, &k,
                 as->edge_threshold, &dev, d_samples, &got))
        return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* plain synchronous copies: caller memory is never page-locked */
    void* const* host = (void* const*)out;
    for (int i = 0; i < BHRT_NFIELDS; i++)
        if (host[i])
            HIP_TRY(hipMemcpy(host[i], ((void**)&dev)[i], k_fsize[i] * (size_t)n,
                              hipMemcpyDeviceToHost));
    if (samples)
        HIP_TRY(hipMemcpy(samples, d_samples, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (info) *info = got;
    return 0;
}
