/*
 * bhrt_api.c -- the device API of libbhrt.so: camera frames and ray arrays traced into device
 * arrays (bhrt_render_frame_device, bhrt_trace_rays_device), the claim order of a frame, the
 * SoA helpers every host-buffer path carves its device arrays with, and the multi-device gather.
 * Host code is C11 over the HIP C runtime API (bhrt_host.h lists the modules).
 */
#define _GNU_SOURCE
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

/* claim order of this thread's next device camera frames (bhrt_set_claim_order): a device
 * permutation of [0, n) on device g_order_dev, used only by bhrt_render_frame_device calls on
 * that device for frames of exactly n rays (never by the chunks of host-buffer frames) */
static __thread const int* g_order;
static __thread int g_order_n, g_order_dev = -1;
int bhrt_set_claim_order(const int* d_order, int n) {
    g_order = NULL;
    g_order_n = 0;
    g_order_dev = -1;
    if (!d_order || n <= 0) return 0;
    const int dev = bhrt_current_device();
    if (dev < 0) {
        set_err("bhrt_set_claim_order: no current HIP device");
        return -1;
    }
    if (bhrt_env_int("BHRT_TRUST_CLAIM_ORDER", 0)) { /* the caller guarantees a permutation */
        g_order = d_order;
        g_order_n = n;
        g_order_dev = dev;
        return 0;
    }
    /* claim_ray indexes the outputs with order[position]: only a permutation is safe */
    int* h = (int*)malloc((size_t)n * sizeof(int));
    unsigned char* seen = (unsigned char*)calloc((size_t)n, 1);
    int ok = h && seen &&
             hipMemcpy(h, d_order, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    for (long i = 0; ok && i < n; i++) {
        if (h[i] < 0 || h[i] >= n || seen[h[i]]) ok = 0;
        else seen[h[i]] = 1;
    }
    free(h);
    free(seen);
    if (!ok) {
        set_err("bhrt_set_claim_order: the order is not a device permutation of [0, %d)", n);
        return -1;
    }
    g_order = d_order;
    g_order_n = n;
    g_order_dev = dev;
    return 0;
}

int bhrt_shard_rows(int H, const bhrt_rows* rows) {
    if (H <= 0) return 0;
    if (!rows || rows->num_shards <= 1) return H;
    if (rows->row_block <= 0 || rows->shard < 0 || rows->shard >= rows->num_shards) return -1;
    int B = rows->row_block, n = 0;
    for (long b = rows->shard; b * B < H; b += rows->num_shards) {
        long hi = (b + 1) * B;
        n += (int)((hi > H ? H : hi) - b * B);
    }
    return n;
}

/* The claim order of a camera launch (geodesic.hip claim_ray): the shard's W x nrows pixels in
 * 64-pixel tiles -- 8x8, else 16x4, else 32x2, the first that divides the shard -- so a
 * wavefront traces a compact patch of the image whose rays live alike. RK4 scenes only: same-box
 * A/B against ray id order (profiles/r03_ab/tiles_v32.txt) C4 -2.1% kernel time, C2 neutral
 * resident but +1.4% synchronous / +1.8% rgba8 host frames (a lone frame's drain is shorter);
 * RKF45 scenes keep id order (C3 +1.5% slower with tiles, C5 neutral). BHRT_TILES=0: ray id
 * order (A/B). */
static void claim_tiles(bhrt_camera_k* k, int W, int nrows) {
    static const int shape[3][2] = {{3, 3}, {4, 2}, {5, 1}}; /* log2 of tile width, height */
    k->tiles_per_row = 0;
    if (bhrt_env_int("BHRT_TILES", 1) == 0) return;
    for (int i = 0; i < 3; i++) {
        const int tw = 1 << shape[i][0], th = 1 << shape[i][1];
        if (W % tw == 0 && nrows % th == 0) {
            k->tile_w_log2 = shape[i][0];
            k->tile_h_log2 = shape[i][1];
            k->tiles_per_row = W / tw;
            k->inv_tiles_per_row = 1.0 / (double)k->tiles_per_row;
            k->ntiles = k->tiles_per_row * (nrows / th);
            k->tile_stride = 0;
            if (bhrt_env_int("BHRT_TILE_SCATTER", 0) && k->ntiles > 2) {
                /* a stride near ntiles / golden ratio, coprime with ntiles: consecutive claims
                 * (a wave's block of tiles) land far apart in the image */
                int st = (int)(k->ntiles * 0.6180339887498949);
                while (st > 1) {
                    int a = st, b = k->ntiles;
                    while (b) {
                        const int t = a % b;
                        a = b;
                        b = t;
                    }
                    if (a == 1) break;
                    st--;
                }
                k->tile_stride = st;
            }
            return;
        }
    }
}

static int launch(devctx_t* c, bhrt_kparams* kp, hipStream_t stream) {
    return bhrt_ctx_launch_fn(c, kp, stream, NULL, NULL);
}

/* use_order: whether the thread's claim order (bhrt_set_claim_order) may apply -- the public
 * device API only; the chunks of host-buffer frames always take the default order */
int bhrt_frame_on_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         const bhrt_rows* rows, IntegrationMethod method, int flags,
                         const bhrt_frame_soa* out, hipStream_t stream, int use_order) {
    if (bhrt_check_scene(bh, cfg) || !cam || !out || W <= 0 || H <= 0) {
        if (!bhrt_err_is_set()) set_err("invalid argument");
        return -1;
    }
    int nrows = bhrt_shard_rows(H, rows);
    if (nrows < 0 || (long)nrows * W > 0x7fffffffL) {
        set_err("invalid row sharding or frame too large (%d x %d)", W, H);
        return -1;
    }
    int dev = bhrt_current_device();
    devctx_t* c = bhrt_ctx_get(dev);
    if (!c) return -1;
    if (bhrt_colour_args_bad(out, (int)method, dk != NULL, bh->spin != 0.0)) return -1;
    if (!stream && bhrt_ctx_streams(c)) return -1;
    void* scratch = bhrt_stream_scratch(c, stream ? stream : c->stream,
                                   (size_t)BHRT_SCRATCH_FIELDS * sizeof(double) *
                                       (size_t)nrows * (size_t)W);
    if (!scratch) return -1;
    bhrt_kparams kp;
    if (bhrt_fill_scene(&kp, bh, dk, cfg, method, flags)) return -1;
    bhrt_fill_camera(&kp, cam, W, H);
    if (rows && rows->num_shards > 1) {
        kp.cam.rows = *rows;
        kp.cam.inv_block = 1.0 / (double)rows->row_block;
    }
    kp.n = nrows * W;
    kp.init = (double*)scratch;
    kp.out = *out;
    if (use_order && g_order && g_order_n == kp.n && g_order_dev == dev) kp.order = g_order;
    else if (method == INTEGRATOR_RK4) claim_tiles(&kp.cam, W, nrows);
    return launch(c, &kp, stream);
}

/* origin: non-NULL when the host knows every ray starts at *origin (shared_origin): the
 * origin's set-up is then done once here, as for a camera frame, and the trace kernel sets each
 * ray up from its direction alone (no k_init table). The rays are d_rays (AoS), or -- with an
 * origin only -- d_rays NULL and d_dirs their packed directions (3 doubles per ray: half the
 * upload of trace_rays_batch's chunks). */
int bhrt_rays_on_device(const Ray* d_rays, const double* d_dirs, int n,
                        const BlackHoleParams* bh, const AccretionDiskParams* dk,
                        const SimulationConfig* cfg, IntegrationMethod method, int flags,
                        const bhrt_frame_soa* out, hipStream_t stream, const Vector3D* origin) {
    if (bhrt_check_scene(bh, cfg) || !(d_rays || (d_dirs && origin)) || !out || n < 0) {
        if (!bhrt_err_is_set()) set_err("invalid argument");
        return -1;
    }
    if (bhrt_colour_args_bad(out, (int)method, dk != NULL, bh->spin != 0.0)) return -1;
    devctx_t* c = bhrt_ctx_get(bhrt_current_device());
    if (!c) return -1;
    if (!stream && bhrt_ctx_streams(c)) return -1;
    void* scratch = bhrt_stream_scratch(c, stream ? stream : c->stream,
                                   (size_t)BHRT_SCRATCH_FIELDS * sizeof(double) * (size_t)n);
    if (!scratch) return -1;
    bhrt_kparams kp;
    if (bhrt_fill_scene(&kp, bh, dk, cfg, method, flags)) return -1;
    kp.src = BHRT_SRC_RAYS;
    kp.rays = d_rays;
    kp.init = (double*)scratch;
    kp.n = n;
    kp.out = *out;
    if (origin && (bhrt_env_int("BHRT_SHARED_ORIGIN", 1) || !d_rays)) {
        bhrt_fill_origin(&kp, origin);
        kp.rays_shared = 1;
        kp.dirs = d_rays ? &d_rays[0].direction.x : d_dirs;
        kp.dir_stride = d_rays ? (int)(sizeof(Ray) / sizeof(double)) : 3;
    }
    return launch(c, &kp, stream);
}

/* the public entry points: the bodies above under the device API's stream rule (context.c
 * bhrt_on_stream), each making its context after its own argument checks */
typedef struct {
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam;
    int W, H;
    const bhrt_rows* rows;
    IntegrationMethod method;
    int flags;
    const bhrt_frame_soa* out;
    const Ray* d_rays;
    int n;
} dev_call;

static int frame_body(devctx_t* c, hipStream_t st, const void* arg) {
    const dev_call* a = (const dev_call*)arg;
    return bhrt_frame_on_device(a->bh, a->dk, a->cfg, a->cam, a->W, a->H, a->rows, a->method,
                                a->flags, a->out, st, 1);
}

int bhrt_render_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                             const bhrt_rows* rows, IntegrationMethod method, int flags,
                             const bhrt_frame_soa* out, void* stream) {
    const dev_call a = {bh, dk, cfg, cam, W, H, rows, method, flags, out, NULL, 0};
    return bhrt_on_stream(NULL, (hipStream_t)stream, frame_body, &a);
}

static int rays_body(devctx_t* c, hipStream_t st, const void* arg) {
    const dev_call* a = (const dev_call*)arg;
    return bhrt_rays_on_device(a->d_rays, NULL, a->n, a->bh, a->dk, a->cfg, a->method, a->flags,
                               a->out, st, NULL);
}

int bhrt_trace_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                           void* stream) {
    const dev_call a = {bh, dk, cfg, NULL, 0, 0, NULL, method, flags, out, d_rays, n};
    return bhrt_on_stream(NULL, (hipStream_t)stream, rays_body, &a);
}

/* ---- host-buffer paths: device SoA block <-> caller SoA ---- */
/* the fields a device SoA needs for the fields `want_in` requests */
bhrt_frame_soa bhrt_device_fields(const bhrt_frame_soa* want_in, int method, int has_disk,
                                  int spin) {
    bhrt_frame_soa want_buf = *want_in;
    if (want_buf.rgb_r || want_buf.rgb_g || want_buf.rgb_b) /* written together */
        want_buf.rgb_r = want_buf.rgb_g = want_buf.rgb_b = (double*)1;
    if ((want_buf.rgb_r || want_buf.rgba32f || want_buf.rgba8) &&
        !bhrt_colour_fused(method, has_disk, spin)) {
        /* the separate colour pass reads these */
        if (!want_buf.result) want_buf.result = (int32_t*)1;
        if (!want_buf.hit_x) want_buf.hit_x = (double*)1;
        if (!want_buf.hit_y) want_buf.hit_y = (double*)1;
    }
    return want_buf;
}

size_t bhrt_soa_bytes(const bhrt_frame_soa* fields, long n) {
    size_t bytes = 0;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (*soa_slot((bhrt_frame_soa*)fields, f)) bytes += align256(k_fsize[f] * n);
    return bytes;
}

/* point dev's fields at consecutive 256-byte-aligned arrays of n elements from *p */
void bhrt_soa_carve(char** p, const bhrt_frame_soa* fields, long n, bhrt_frame_soa* dev) {
    memset(dev, 0, sizeof *dev);
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (*soa_slot((bhrt_frame_soa*)fields, f)) {
            *soa_slot(dev, f) = *p;
            *p += align256(k_fsize[f] * n);
        }
}

/* ---- multi-device device frames (bhrt_render_frame_gather) ---- */
#define BHRT_GATHER_MAX_SHARDS 64

static int lazy_event(hipEvent_t* e) {
    if (*e) return 0;
    HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return 0;
}

/* shard s's rows of field f (element size fs) from its shard buffer src into their image rows
 * of dst: the shard's full 8-row blocks are one strided 2-D copy (block j -> image block
 * j * S + s), the frame's last, partial block one more copy. Peer memory goes over xGMI. */
static int gather_field(char* dst, const char* src, size_t fs, int W, int H, int B, int s, int S,
                        int src_dev, devctx_t* root, hipStream_t rs) {
    const size_t wb = fs * (size_t)W, blk = wb * (size_t)B;
    const int nbf = H / B; /* full blocks of the image */
    const int nfull = nbf > s ? (nbf - 1 - s) / S + 1 : 0;
    const int peer = src_dev != root->device;
    if (peer && !(root->peer_on >> src_dev & 1ull)) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, root->device, src_dev) == hipSuccess && can) {
            hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) root->peer_on |= 1ull << src_dev;
            (void)hipGetLastError();
        }
    }
    if (!peer || (root->peer_on >> src_dev & 1ull)) {
        if (nfull > 0)
            HIP_TRY(hipMemcpy2DAsync(dst + (size_t)s * blk, (size_t)S * blk, src, blk, blk,
                                     (size_t)nfull, hipMemcpyDeviceToDevice, rs));
    } else { /* no peer mapping: one runtime peer copy per block */
        for (int j = 0; j < nfull; j++)
            HIP_TRY(hipMemcpyPeerAsync(dst + ((size_t)j * S + s) * blk, root->device,
                                       src + (size_t)j * blk, src_dev, blk, rs));
    }
    if (H % B && nbf % S == s) { /* the partial last block is this shard's */
        const size_t rows = (size_t)(H - nbf * B), off = (size_t)(nbf / S) * blk;
        if (!peer || (root->peer_on >> src_dev & 1ull))
            HIP_TRY(hipMemcpyAsync(dst + (size_t)nbf * blk, src + off, rows * wb,
                                   hipMemcpyDeviceToDevice, rs));
        else
            HIP_TRY(hipMemcpyPeerAsync(dst + (size_t)nbf * blk, root->device, src + off, src_dev,
                                       rows * wb, rs));
    }
    return 0;
}

static int gather_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                        const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                        IntegrationMethod method, int flags, const bhrt_frame_soa* out, int ndev,
                        int S, int total, int root, devctx_t* rc, hipStream_t rs) {
    const int B = 8;
    for (int k = 0; k < (S == 1 ? 1 : ndev); k++) /* a sky map serves its own device only */
        if (bhrt_sky_check(flags, (root + k) % total)) return -1;
    if (S == 1)
        return bhrt_frame_on_device(bh, dk, cfg, cam, W, H, NULL, method, flags, out, rs, 0);
    const bhrt_frame_soa fields = bhrt_device_fields(out, (int)method, dk != NULL, bh->spin != 0.0);
    bhrt_frame_soa shard_soa[BHRT_GATHER_MAX_SHARDS];
    int rc_all = 0;
    for (int k = 0; k < ndev && rc_all == 0; k++) { /* every device renders its shards */
        const int d = (root + k) % total;
        devctx_t* c = bhrt_ctx_get(d);
        if (!c || hipSetDevice(d) != hipSuccess) {
            if (c) set_err("hipSetDevice(%d) failed", d);
            rc_all = -1;
            break;
        }
        if (k > 0 && bhrt_ctx_streams(c)) {
            rc_all = -1;
            break;
        }
        hipStream_t st = k == 0 ? rs : c->stream;
        size_t bytes = 0;
        for (int s = k; s < S; s += ndev) {
            const bhrt_rows r = {B, s, S};
            bytes += bhrt_soa_bytes(&fields, (long)bhrt_shard_rows(H, &r) * W);
        }
        /* the last gather's copies must have read this device's shard buffers */
        if (c->g_wait_pending && hipStreamWaitEvent(st, c->g_wait, 0) != hipSuccess) {
            set_err("hipStreamWaitEvent failed");
            rc_all = -1;
            break;
        }
        /* ... and before the buffers are freed to grow: those copies run on the ROOT's stream,
         * and hipFree drains only this device's queues (the stream wait above orders later GPU
         * work, not a host-side free) */
        const size_t need = bytes ? bytes : 256;
        if (c->g_wait_pending && c->cap_gather < need) {
            if (hipEventSynchronize(c->g_wait) != hipSuccess) {
                set_err("hipEventSynchronize failed");
                rc_all = -1;
                break;
            }
            c->g_wait_pending = 0;
        }
        if (bhrt_ensure(&c->d_gather, &c->cap_gather, need, 0) || lazy_event(&c->g_done) ||
            lazy_event(&c->g_copied)) {
            rc_all = -1;
            break;
        }
        char* p = (char*)c->d_gather;
        for (int s = k; s < S && rc_all == 0; s += ndev) {
            const bhrt_rows r = {B, s, S};
            bhrt_soa_carve(&p, &fields, (long)bhrt_shard_rows(H, &r) * W, &shard_soa[s]);
            rc_all = bhrt_frame_on_device(bh, dk, cfg, cam, W, H, &r, method, flags, &shard_soa[s],
                                         st, 0);
        }
        if (rc_all == 0 && k > 0 && hipEventRecord(c->g_done, st) != hipSuccess) {
            set_err("hipEventRecord failed");
            rc_all = -1;
        }
    }
    if (hipSetDevice(root) != hipSuccess) {
        set_err("hipSetDevice(%d) failed", root);
        return -1;
    }
    if (rc_all) return -1;
    for (int k = 1; k < ndev; k++) /* the root's copies follow every peer's render */
        HIP_TRY(hipStreamWaitEvent(rs, bhrt_ctx_get((root + k) % total)->g_done, 0));
    for (int s = 0; s < S; s++) {
        const int d = (root + s % ndev) % total;
        for (int f = 0; f < BHRT_NFIELDS; f++) {
            char* dst = (char*)*soa_slot((bhrt_frame_soa*)out, f);
            const char* src = (const char*)*soa_slot(&shard_soa[s], f);
            if (dst && src && gather_field(dst, src, k_fsize[f], W, H, B, s, S, d, rc, rs))
                return -1;
        }
    }
    HIP_TRY(hipEventRecord(rc->g_copied, rs));
    for (int k = 0; k < ndev; k++) {
        devctx_t* c = bhrt_ctx_get((root + k) % total);
        c->g_wait = rc->g_copied;
        c->g_wait_pending = 1;
    }
    return 0;
}

int bhrt_render_frame_gather(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                             IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                             int ndev_req, int shards_req, void* stream) {
    if (bhrt_check_scene(bh, cfg) || !cam || !out || W <= 0 || H <= 0) {
        if (!bhrt_err_is_set()) set_err("invalid argument");
        return -1;
    }
    if ((long)W * H > 0x7fffffffL) {
        set_err("frame too large (%d x %d)", W, H);
        return -1;
    }
    if ((out->rgb_r || out->rgb_g || out->rgb_b) && !(out->rgb_r && out->rgb_g && out->rgb_b)) {
        set_err("rgb output needs all of rgb_r/g/b");
        return -1;
    }
    const int total = bhrt_device_count();
    if (total <= 0) {
        set_err("no HIP device available (libbhrt has no CPU path)");
        return -1;
    }
    const int root = bhrt_current_device();
    if (root < 0 || root >= total) {
        set_err("the current device %d is not one libbhrt drives", root);
        return -1;
    }
    const int B = 8;
    int ndev = ndev_req > 0 && ndev_req < total ? ndev_req : total;
    int S = shards_req > 0 ? shards_req : ndev;
    if (S > BHRT_GATHER_MAX_SHARDS) S = BHRT_GATHER_MAX_SHARDS;
    while (S > 1 && H < S * B) S--; /* every shard at least one row block */
    if (ndev > S) ndev = S;
    devctx_t* rc = bhrt_ctx_get(root);
    if (!rc || (!stream && bhrt_ctx_streams(rc))) return -1;
    hipStream_t rs = stream ? (hipStream_t)stream : rc->stream;
    /* NULL stream: the root's work -- the only writes into device_out -- is ordered like the
     * legacy default stream's (bhrt_null_fence); the peers render into libbhrt's own buffers */
    const int fence = !stream && !bhrt_null_unordered();
    if (fence && bhrt_null_fence(rc, 0)) return -1;
    const int e = gather_frame(bh, dk, cfg, cam, W, H, method, flags, out, ndev, S, total, root,
                               rc, rs);
    if (fence && hipSetDevice(root) == hipSuccess && bhrt_null_fence(rc, 1)) return -1;
    return e;
}
