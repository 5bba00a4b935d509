/*
 * host_frames.c -- the host-buffer paths: frames traced in chunks with up to three frames in
 * flight (bhrt_render_frame[_async], bhrt_frame_wait), the readback of a device SoA into the
 * caller's arrays with its un-permuting copy loop, and bhrt_trace_rays.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "bhrt_host.h"

/* whether rays[0, n) all start at rays[0].origin (bit for bit) */
static int shared_origin(const Ray* rays, long n, int nthreads) {
    if (n <= 0) return 0;
    const Vector3D o = rays[0].origin;
    int diff = 0;
#pragma omp parallel for schedule(static) reduction(| : diff) num_threads(nthreads) if (n >= 65536)
    for (long i = 1; i < n; i++)
        diff |= memcmp(&rays[i].origin, &o, sizeof o) != 0;
    return !diff;
}

/* carve a device SoA for n rays out of c->d_soa, for the fields `want` requests */
static int device_soa(devctx_t* c, long n, const bhrt_frame_soa* want_in, int method,
                      int has_disk, int spin, bhrt_frame_soa* dev) {
    const bhrt_frame_soa fields = bhrt_device_fields(want_in, method, has_disk, spin);
    const size_t bytes = bhrt_soa_bytes(&fields, n);
    if (bhrt_ensure(&c->d_soa, &c->cap_soa, bytes ? bytes : 256, 0)) return -1;
    char* p = (char*)c->d_soa;
    bhrt_soa_carve(&p, &fields, n, dev);
    return 0;
}

/* only the fields the caller asked for (the device may hold extra ones, e.g. the hit point
 * the colour pass reads) */
#define WANTED(j, host, f) \
    (*soa_slot((bhrt_frame_soa*)&(j)->dev, f) && *soa_slot((bhrt_frame_soa*)(host), f))

static size_t wanted_bytes(const shard_job* j, const bhrt_frame_soa* host) {
    size_t bytes = 0;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (WANTED(j, host, f)) bytes += k_fsize[f] * (size_t)j->n;
    return bytes;
}

/* enqueue the D2H of a shard's wanted fields into pinned `stage` on stream st. With `parts`
 * events, the fields are cut into up to BHRT_COPY_PARTS consecutive groups of about equal bytes,
 * part q's event is recorded once its copies are queued and part_end[q] = the field after it
 * (*nparts = the parts used): the host can un-permute a part while the next one copies. */
static int readback_issue(shard_job* j, const bhrt_frame_soa* host, char* stage, hipStream_t st,
                          hipEvent_t* parts, unsigned char* part_end, int* nparts) {
    const size_t total = wanted_bytes(j, host);
    size_t off = 0;
    int q = 0, last = -1;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (WANTED(j, host, f)) last = f;
    for (int f = 0; f < BHRT_NFIELDS; f++) {
        if (!WANTED(j, host, f)) continue;
        HIP_TRY(hipMemcpyAsync(stage + off, *soa_slot(&j->dev, f), k_fsize[f] * (size_t)j->n,
                               hipMemcpyDeviceToHost, st));
        off += k_fsize[f] * (size_t)j->n;
        if (parts && (f == last || (q < BHRT_COPY_PARTS - 1 &&
                                    off * BHRT_COPY_PARTS >= total * (size_t)(q + 1)))) {
            HIP_TRY(hipEventRecord(parts[q], st));
            part_end[q++] = (unsigned char)(f + 1);
        }
    }
    if (nparts) *nparts = q;
    return 0;
}

/* copy a landed shard from `stage` into `host`, un-permuting cyclic row blocks. A C2 frame
 * is ~200 MB of fields; one thread copies it at a fraction of the host's memory bandwidth, so
 * the rows of large shards are split over OpenMP threads (BHRT_HOST_THREADS; default 16, at
 * most the processors OpenMP sees: C2 three frames in flight 210 Mrays/s with 8, 221 with 16,
 * profiles/r02_ab_v24.txt). */
int bhrt_host_threads(void) {
    const char* e = getenv("BHRT_HOST_THREADS");
    int t = 16;
    if (e) {
        t = atoi(e);
    } else {
#ifdef _OPENMP
        const int np = omp_get_num_procs();
        if (np >= 1 && np < t) t = np;
#endif
    }
    return t < 1 ? 1 : (t > 64 ? 64 : t);
}

static void readback_finish(const shard_job* j, const bhrt_frame_soa* host, const char* stage,
                            int W, const bhrt_rows* rows, int f_lo, int f_hi) {
    /* every wanted field of the chunk as pieces of <= 1 MB (one image row at a time when the
     * rows are permuted), all copied in ONE parallel loop: a C2 chunk is ~50 MB, and a single
     * thread moves pinned staging at ~16 GB/s, which made the copies, not the GPU, the bound of
     * frames in flight */
    const int nthreads = bhrt_host_threads();
    const int permute = rows && rows->num_shards > 1 && W > 0;
    const size_t piece = (size_t)1 << 20;
    long total_pieces = 0, npieces[BHRT_NFIELDS];
    size_t off[BHRT_NFIELDS], bytes_all = 0;
    size_t o = 0;
    for (int f = 0; f < BHRT_NFIELDS; f++) {
        npieces[f] = 0;
        off[f] = o;
        if (!WANTED(j, host, f)) continue;
        const size_t total = k_fsize[f] * (size_t)j->n;
        o += total;
        if (f < f_lo || f >= f_hi) continue; /* (its bytes still precede later fields in stage) */
        npieces[f] = permute ? j->n / W : (long)((total + piece - 1) / piece);
        total_pieces += npieces[f];
        bytes_all += total;
    }
    const int big = bytes_all >= ((size_t)1 << 22);
#pragma omp parallel for schedule(static) num_threads(nthreads) if (big)
    for (long q = 0; q < total_pieces; q++) {
        long r = q;
        int f = 0;
        while (r >= npieces[f]) r -= npieces[f++];
        char* dst = (char*)*soa_slot((bhrt_frame_soa*)host, f);
        const char* src = stage + off[f];
        const size_t fs = k_fsize[f];
        if (permute) { /* local row r is image row g */
            const size_t row_bytes = fs * (size_t)W;
            const long B = rows->row_block, S = rows->num_shards, sh = rows->shard;
            const long g = ((r / B) * S + sh) * B + r % B;
            memcpy(dst + row_bytes * (size_t)g, src + row_bytes * (size_t)r, row_bytes);
        } else {
            const size_t total = fs * (size_t)j->n, a0 = piece * (size_t)r;
            memcpy(dst + a0, src + a0, total - a0 < piece ? total - a0 : piece);
        }
    }
}

/* copy a finished device SoA back into `host` (synchronous) */
static int readback(shard_job* j, const bhrt_frame_soa* host, int W, const bhrt_rows* rows) {
    devctx_t* c = j->c;
    HIP_TRY(hipSetDevice(c->device));
    if (bhrt_ctx_streams(c)) return -1;
    const size_t bytes = wanted_bytes(j, host);
    if (bhrt_ensure(&c->h_stage, &c->cap_stage, bytes ? bytes : 64, 1)) return -1;
    if (readback_issue(j, host, (char*)c->h_stage, c->stream, NULL, NULL, NULL)) return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    readback_finish(j, host, (const char*)c->h_stage, W, rows, 0, BHRT_NFIELDS);
    return 0;
}

/* ---- host-buffer frames (bhrt_render_frame[_async]) ---- */
/* A frame is traced in K chunks per device -- cyclic row-block shards k*ndev + d of K*ndev, so
 * every chunk carries the same mix of work -- alternating between two trace streams, so a
 * chunk's workgroups fill the CUs its predecessor's tail (the longest rays) frees. Each
 * finished chunk is copied on the copy stream into pinned staging while later chunks trace,
 * and un-permuted into the caller's arrays by OpenMP threads when the frame is waited for
 * (the next frames in flight keep the GPU busy meanwhile). The caller's arrays are never
 * page-locked: libbhrt registers no caller memory (DESIGN.md §4 "Host-buffer frames" -- the
 * round-3 removal of the registered path and why). */

typedef struct {
    int active, ticket, ndev, K, shards, W, H;
    unsigned long long last_use;
    int timing;             /* BHRT_HOST_TIMING: print where the frame's time went (device 0) */
    hipEvent_t t_ev[2 + 2 * BHRT_MAX_CHUNKS];
    double t_host[4];
    bhrt_frame_soa host;
    shard_job jobs[BHRT_MAX_CHUNKS][BHRT_MAX_DEV];
    bhrt_rows rows[BHRT_MAX_CHUNKS][BHRT_MAX_DEV];
    size_t stage_off[BHRT_MAX_CHUNKS][BHRT_MAX_DEV];
    int nparts[BHRT_MAX_CHUNKS][BHRT_MAX_DEV];   /* readback_issue's parts of each chunk */
    unsigned char part_end[BHRT_MAX_CHUNKS][BHRT_MAX_DEV][BHRT_COPY_PARTS];
} host_frame;

static _Thread_local host_frame* g_frames; /* [BHRT_FRAME_SLOTS], allocated on first use */
static _Thread_local int g_next_ticket;
static _Thread_local unsigned long long g_frame_clock;
/* frames a later issue completed implicitly (frame_slot), kept for their own bhrt_frame_wait:
 * a ring of the last BHRT_REAPED results, so reaping one slot again before the caller waited
 * on the first ticket does not lose that result */
#define BHRT_REAPED 32
static _Thread_local struct {
    int ticket, rc;
} g_reaped[BHRT_REAPED];
static _Thread_local int g_reaped_next;

/* Chunks per device: each chunk's copy overlaps the tracing of the next, so only the last
 * chunk's copy follows the trace; but a chunk of C2 is traced by a full-chip persistent grid,
 * and below ~2 rays per resident lane a chunk is all tail. C2 (2 M rays), same box, ms per
 * frame for 1/2/3/4/8 chunks: synchronous 16.9/17.0/14.4/11.5-11.9/19.1, three frames in
 * flight 1 chunk 12.2-12.6, 4 chunks 10.3-10.4 (profiles/r02_host_path.txt). */
static int frame_chunks(int ndev, int W, int H, int block) {
    const long per_dev = (long)W * H / ndev;
    int K = per_dev >= (1L << 20) ? 4 : (per_dev >= (1L << 18) ? 2 : 1);
    const char* env = getenv("BHRT_HOST_CHUNKS");
    if (env && atoi(env) >= 1 && atoi(env) <= BHRT_MAX_CHUNKS) K = atoi(env);
    while (K > 1 && H < K * ndev * block) K--;
    return K;
}

/* wait for every copy a frame queued, then un-permute its staged chunks into the caller arrays */
static int frame_complete(host_frame* f) {
    const int slot = (int)(f - g_frames);
    int rc = 0;
    struct timespec tw0;
    clock_gettime(CLOCK_MONOTONIC, &tw0);
    for (int k = 0; k < f->K && rc == 0; k++)
        for (int d = 0; d < f->ndev && rc == 0; d++) {
            devctx_t* c = f->jobs[k][d].c;
            if (hipSetDevice(d) != hipSuccess) {
                set_err("frame %d: hipSetDevice(%d) failed", f->ticket, d);
                rc = -1;
                break;
            }
            /* each part of the chunk is un-permuted as soon as it has landed, while the next
             * part still copies (a synchronous frame's last chunk: copy and host copy overlap) */
            const int np = f->jobs[k][d].n > 0 ? f->nparts[k][d] : 0;
            for (int q = 0, lo = 0; q < np && rc == 0; lo = f->part_end[k][d][q++]) {
                if (hipEventSynchronize(c->fr[slot].part[k][q]) != hipSuccess) {
                    set_err("frame %d: waiting for chunk %d of device %d failed", f->ticket, k, d);
                    rc = -1;
                    break;
                }
                readback_finish(&f->jobs[k][d], &f->host,
                                (const char*)c->fr[slot].h_stage + f->stage_off[k][d], f->W,
                                f->shards > 1 ? &f->rows[k][d] : NULL, lo, f->part_end[k][d][q]);
            }
            if (rc == 0 && hipEventSynchronize(c->fr[slot].copied[k]) != hipSuccess) {
                set_err("frame %d: waiting for chunk %d of device %d failed", f->ticket, k, d);
                rc = -1;
            }
        }
    if (f->timing && rc == 0) {
        struct timespec tw1;
        clock_gettime(CLOCK_MONOTONIC, &tw1);
        float tr[BHRT_MAX_CHUNKS], cp[BHRT_MAX_CHUNKS];
        for (int k = 0; k < f->K; k++) {
            (void)hipEventElapsedTime(&tr[k], f->t_ev[0], f->t_ev[2 + 2 * k]);
            (void)hipEventElapsedTime(&cp[k], f->t_ev[0], f->t_ev[3 + 2 * k]);
        }
        fprintf(stderr, "libbhrt frame %d (K=%d): enqueue %.2f ms, staging %.2f ms, copies "
                "queued %.2f ms, wait %.2f ms |", f->ticket, f->K,
                f->t_host[0], f->t_host[1], f->t_host[2],
                (tw1.tv_sec - tw0.tv_sec) * 1e3 + (tw1.tv_nsec - tw0.tv_nsec) * 1e-6);
        for (int k = 0; k < f->K; k++) fprintf(stderr, " chunk %d traced %.2f copied %.2f", k, tr[k], cp[k]);
        fprintf(stderr, "\n");
    }
    /* a failed wait leaves later chunks' copies queued into the slot's staging: drain them
     * before the slot can be reused (bhrt_ensure() may reallocate what a DMA still targets) */
    if (rc != 0) bhrt_drain_devices(f->ndev);
    return rc;
}

int bhrt_frame_wait(int ticket) {
    if (!g_frames || ticket <= 0) {
        set_err("no such frame ticket %d", ticket);
        return -1;
    }
    for (int s = 0; s < BHRT_FRAME_SLOTS; s++) {
        host_frame* f = &g_frames[s];
        if (f->active && f->ticket == ticket) {
            f->active = 0;
            return frame_complete(f);
        }
    }
    for (int i = 0; i < BHRT_REAPED; i++)
        if (g_reaped[i].ticket == ticket) { /* completed when a later issue needed its slot */
            g_reaped[i].ticket = 0;
            if (g_reaped[i].rc) set_err("frame %d failed", ticket);
            return g_reaped[i].rc;
        }
    set_err("frame ticket %d is not in flight", ticket);
    return -1;
}

/* The slot for a new frame: an idle slot, the most recently used one first (its buffers are
 * warm: a caller of the synchronous API keeps reusing ONE slot's device SoA and pinned
 * staging); with every slot in flight, the oldest frame is completed first and its result kept
 * for its own bhrt_frame_wait. */
static host_frame* frame_slot(void) {
    host_frame* best = NULL;
    for (int s = 0; s < BHRT_FRAME_SLOTS; s++) {
        host_frame* f = &g_frames[s];
        if (!f->active && (!best || f->last_use > best->last_use)) best = f;
    }
    if (best) return best;
    for (int s = 0; s < BHRT_FRAME_SLOTS; s++)
        if (!best || g_frames[s].ticket < best->ticket) best = &g_frames[s];
    best->active = 0;
    const int rc = frame_complete(best);
    g_reaped[g_reaped_next].ticket = best->ticket;
    g_reaped[g_reaped_next].rc = rc;
    g_reaped_next = (g_reaped_next + 1) % BHRT_REAPED;
    return best;
}

/* A frame whose issue failed part way: its launches and copies may still be queued on the
 * slot's device buffers and pinned staging, so drain every stream it used before the caller
 * sees the error (a later issue may then reallocate the slot's buffers). */
static void frame_abort(host_frame* f, int ndev) {
    bhrt_drain_devices(ndev);
    f->active = 0;
}

static int frame_enqueue(host_frame* f, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam,
                         IntegrationMethod method, int flags) {
    const int slot = (int)(f - g_frames), ticket = f->ticket, ndev = f->ndev, K = f->K,
              shards = f->shards, W = f->W, H = f->H, block = 8;
    const bhrt_frame_soa* host = &f->host;
    struct timespec th[4];
    clock_gettime(CLOCK_MONOTONIC, &th[0]);
    if (f->timing && !f->t_ev[0]) {
        HIP_TRY(hipSetDevice(0));
        for (int i = 0; i < 2 + 2 * BHRT_MAX_CHUNKS; i++) HIP_TRY(hipEventCreate(&f->t_ev[i]));
    }
    const bhrt_frame_soa fields = bhrt_device_fields(host, (int)method, dk != NULL, bh->spin != 0.0);
    for (int d = 0; d < ndev; d++) { /* device buffers: every chunk of device d */
        devctx_t* c = bhrt_ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (bhrt_ctx_streams(c)) return -1;
        size_t dev_bytes = 0;
        for (int k = 0; k < K; k++) {
            bhrt_rows* r = &f->rows[k][d];
            r->row_block = block;
            r->shard = k * ndev + d;
            r->num_shards = shards;
            f->jobs[k][d].c = c;
            f->jobs[k][d].n = shards > 1 ? (long)bhrt_shard_rows(H, r) * W : (long)W * H;
            dev_bytes += bhrt_soa_bytes(&fields, f->jobs[k][d].n);
        }
        if (bhrt_ensure(&c->fr[slot].d_soa, &c->fr[slot].cap_soa, dev_bytes ? dev_bytes : 256, 0))
            return -1;
        char* p = (char*)c->fr[slot].d_soa;
        for (int k = 0; k < K; k++) bhrt_soa_carve(&p, &fields, f->jobs[k][d].n, &f->jobs[k][d].dev);
    }
    if (f->timing) { /* time origin: when the frame's first chunk is queued */
        HIP_TRY(hipSetDevice(0));
        HIP_TRY(hipEventRecord(f->t_ev[0], (ticket & 1) ? f->jobs[0][0].c->stream2
                                                          : f->jobs[0][0].c->stream));
    }
    for (int k = 0; k < K; k++) /* trace every chunk; consecutive chunks and frames alternate */
        for (int d = 0; d < ndev; d++) {
            devctx_t* c = f->jobs[k][d].c;
            hipStream_t st = ((k + ticket) & 1) ? c->stream2 : c->stream;
            HIP_TRY(hipSetDevice(d));
            if (f->jobs[k][d].n > 0 &&
                bhrt_frame_on_device(bh, dk, cfg, cam, W, H, shards > 1 ? &f->rows[k][d] : NULL,
                                    method, flags, &f->jobs[k][d].dev, st, 0))
                return -1;
            HIP_TRY(hipEventRecord(c->fr[slot].done[k], st));
            if (f->timing && d == 0) HIP_TRY(hipEventRecord(f->t_ev[2 + 2 * k], st));
        }
    clock_gettime(CLOCK_MONOTONIC, &th[1]);
    for (int d = 0; d < ndev; d++) { /* pinned staging: every chunk of device d */
        devctx_t* c = f->jobs[0][d].c;
        size_t host_bytes = 0;
        for (int k = 0; k < K; k++) {
            f->stage_off[k][d] = host_bytes;
            host_bytes += wanted_bytes(&f->jobs[k][d], host);
        }
        HIP_TRY(hipSetDevice(d));
        if (bhrt_ensure(&c->fr[slot].h_stage, &c->fr[slot].cap_stage, host_bytes ? host_bytes : 64, 1))
            return -1;
    }
    clock_gettime(CLOCK_MONOTONIC, &th[2]);
    for (int k = 0; k < K; k++) /* each chunk's copy queued behind its trace */
        for (int d = 0; d < ndev; d++) {
            devctx_t* c = f->jobs[k][d].c;
            HIP_TRY(hipSetDevice(d));
            HIP_TRY(hipStreamWaitEvent(c->copy, c->fr[slot].done[k], 0));
            f->nparts[k][d] = 0;
            if (f->jobs[k][d].n > 0 &&
                readback_issue(&f->jobs[k][d], host, (char*)c->fr[slot].h_stage + f->stage_off[k][d],
                               c->copy, c->fr[slot].part[k], f->part_end[k][d], &f->nparts[k][d]))
                return -1;
            HIP_TRY(hipEventRecord(c->fr[slot].copied[k], c->copy));
            if (f->timing && d == 0) HIP_TRY(hipEventRecord(f->t_ev[3 + 2 * k], c->copy));
        }
    clock_gettime(CLOCK_MONOTONIC, &th[3]);
    for (int i = 0; i < 3; i++)
        f->t_host[i] = (th[i + 1].tv_sec - th[i].tv_sec) * 1e3 + (th[i + 1].tv_nsec - th[i].tv_nsec) * 1e-6;
    return 0;
}

static int render_frame_issue(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                              const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                              IntegrationMethod method, int flags, const bhrt_frame_soa* host,
                              int* ticket_out) {
    if (ticket_out) *ticket_out = 0;
    if (bhrt_check_scene(bh, cfg) || !cam || !host || W <= 0 || H <= 0) {
        if (!bhrt_err_is_set()) set_err("invalid argument");
        return -1;
    }
    int ndev = bhrt_device_count();
    if (ndev <= 0) {
        set_err("no HIP device available (libbhrt has no CPU path)");
        return -1;
    }
    if (!g_frames && !(g_frames = (host_frame*)calloc(BHRT_FRAME_SLOTS, sizeof(host_frame)))) {
        set_err("host allocation failed");
        return -1;
    }
    host_frame* f = frame_slot();
    const int block = 8;
    if (ndev > 1 && H < ndev * block) ndev = 1;
    const int K = frame_chunks(ndev, W, H, block);
    f->ticket = ++g_next_ticket;
    f->last_use = ++g_frame_clock;
    f->ndev = ndev;
    f->K = K;
    f->shards = K * ndev;
    f->W = W;
    f->H = H;
    f->host = *host;
    f->timing = getenv("BHRT_HOST_TIMING") != NULL;
    for (int d = 0; d < ndev; d++) /* a sky map serves its own device only: before any launch */
        if (bhrt_sky_check(flags, d)) return -1;
    if (frame_enqueue(f, bh, dk, cfg, cam, method, flags)) {
        frame_abort(f, ndev);
        return -1;
    }
    f->active = 1;
    if (ticket_out) *ticket_out = f->ticket;
    return 0;
}

int bhrt_render_frame_async(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                            const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                            IntegrationMethod method, int flags, const bhrt_frame_soa* host,
                            int* ticket) {
    return render_frame_issue(bh, dk, cfg, cam, W, H, method, flags, host, ticket);
}

int bhrt_render_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                      const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                      IntegrationMethod method, int flags, const bhrt_frame_soa* host) {
    int ticket = 0;
    if (render_frame_issue(bh, dk, cfg, cam, W, H, method, flags, host, &ticket)) return -1;
    return bhrt_frame_wait(ticket);
}

int bhrt_trace_rays(const Ray* rays, int n, const BlackHoleParams* bh,
                    const AccretionDiskParams* dk, const SimulationConfig* cfg,
                    IntegrationMethod method, int flags, const bhrt_frame_soa* host) {
    if (bhrt_check_scene(bh, cfg) || !rays || !host || n < 0) {
        if (!bhrt_err_is_set()) set_err("invalid argument");
        return -1;
    }
    if (n == 0) return 0;
    int ndev = bhrt_device_count();
    if (ndev <= 0) {
        set_err("no HIP device available (libbhrt has no CPU path)");
        return -1;
    }
    if (n < 4096 * ndev) ndev = 1; /* small batches: one device, one launch */
    for (int d = 0; d < ndev; d++) /* a sky map serves its own device only: before any launch */
        if (bhrt_sky_check(flags, d)) return -1;
    shard_job jobs[BHRT_MAX_DEV];
    long base[BHRT_MAX_DEV + 1];
    for (int d = 0; d <= ndev; d++) base[d] = (long)n * d / ndev;
    for (int d = 0; d < ndev; d++) {
        devctx_t* c = bhrt_ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (bhrt_ctx_streams(c)) return -1;
        long m = base[d + 1] - base[d];
        jobs[d].c = c;
        jobs[d].n = m;
        if (bhrt_ensure(&c->d_rays, &c->cap_rays, (size_t)m * sizeof(Ray), 0)) return -1;
        if (device_soa(c, m, host, (int)method, dk != NULL, bh->spin != 0.0, &jobs[d].dev)) return -1;
        HIP_TRY(hipMemcpyAsync(c->d_rays, rays + base[d], (size_t)m * sizeof(Ray),
                               hipMemcpyHostToDevice, c->stream));
        const int shared = shared_origin(rays + base[d], m, bhrt_host_threads());
        if (bhrt_rays_on_device((const Ray*)c->d_rays, NULL, (int)m, bh, dk, cfg, method, flags,
                              &jobs[d].dev, c->stream, shared ? &rays[base[d]].origin : NULL))
            return -1;
    }
    for (int d = 0; d < ndev; d++) {
        bhrt_frame_soa h = *host;
        for (int f = 0; f < BHRT_NFIELDS; f++) {
            char** s = (char**)soa_slot(&h, f);
            if (*s) *s += k_fsize[f] * (size_t)base[d];
        }
        if (readback(&jobs[d], &h, 0, NULL)) return -1;
    }
    return 0;
}

/* ---- recorded paths back to the caller (paths.c bhrt_trace_paths, kerr_paths.c) ---- */
/* A copy call's fixed cost, as the bytes a transfer moves meanwhile (about 10 us at the rate of
 * a copy into pageable memory); BHRT_PATHS_COPY_CALL_BYTES overrides it (tests, A/B). */
static size_t copy_call_bytes(void) {
    const char* e = getenv("BHRT_PATHS_COPY_CALL_BYTES");
    return e ? (size_t)strtoull(e, NULL, 10) : (size_t)131072;
}

/* Rows of `elem`-byte points back to the caller, count[i] points of ray i and nothing beyond
 * them. Decided by total bytes: the whole rectangle moves n * P * elem bytes in one call (into a
 * host staging block, the stored points then copied row by row: the caller's tails must keep what
 * they hold); the ragged form moves only sum(count) * elem bytes but in one call per ray, each
 * costing copy_call_bytes() more. The rectangle is taken when it is no more than the ragged total.
 * A batch whose every row is full is its rectangle: one copy straight into the caller's array. */
int bhrt_rows_back(void* host, const void* dev, const int32_t* count, int n, size_t P,
                   size_t elem) {
    size_t total = 0;
    for (int i = 0; i < n; i++) total += (size_t)count[i];
    const size_t rect = (size_t)n * P * elem;
    if (total == (size_t)n * P) {
        HIP_TRY(hipMemcpy(host, dev, rect, hipMemcpyDeviceToHost));
        return 0;
    }
    if (rect <= total * elem + (size_t)n * copy_call_bytes()) {
        char* stage = (char*)malloc(rect);
        if (stage) {
            if (hipMemcpy(stage, dev, rect, hipMemcpyDeviceToHost) != hipSuccess) {
                free(stage);
                bhrt_set_err("paths: readback failed: %s", hipGetErrorString(hipGetLastError()));
                return -1;
            }
            for (int i = 0; i < n; i++)
                memcpy((char*)host + (size_t)i * P * elem, stage + (size_t)i * P * elem,
                       (size_t)count[i] * elem);
            free(stage);
            return 0;
        }
        /* (no memory for the staging block: the ragged form needs none) */
    }
    for (int i = 0; i < n; i++)
        if (count[i] > 0)
            HIP_TRY(hipMemcpy((char*)host + (size_t)i * P * elem,
                              (const char*)dev + (size_t)i * P * elem, (size_t)count[i] * elem,
                              hipMemcpyDeviceToHost));
    return 0;
}
