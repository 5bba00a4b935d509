/*
 * batch.c -- the drop-in trace_ray / trace_rays_batch: rays into RayTraceHit[]. Large batches
 * are pipelined in chunks per device (upload, trace, download and pack overlap); the staging and
 * packing loops stay here with the helpers they inline.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "bhrt_host.h"

/* ======================================================================================= */
/* drop-in ray tracing entry points                                                        */
/* ======================================================================================= */

/* trace rays into RayTraceHit[], writing exactly the fields trace_ray writes
 * (raytracer.c:299-333, 728-753) */
/* pack one traced range into the reference's RayTraceHit (fill_hit_info, raytracer.c:299-333,
 * and trace_ray's disk branch :728-753): only the fields the reference writes */
static inline void pack_one(RayTraceHit* h, const bhrt_frame_soa* s, long i) {
    h->result = (RayTraceResult)s->result[i];
    h->steps = s->steps[i];
    h->hit_position.x = s->hit_x[i];
    h->hit_position.y = s->hit_y[i];
    h->hit_position.z = s->hit_z[i];
    h->distance = s->distance[i];
    h->time_dilation = s->time_dilation[i];
    if (h->result == RAY_MAX_DISTANCE) {
        h->sky_direction.x = s->sky_x[i];
        h->sky_direction.y = s->sky_y[i];
        h->sky_direction.z = s->sky_z[i];
    }
}

static void pack_hits(RayTraceHit* hits, long n, const bhrt_frame_soa* s, int nthreads) {
#pragma omp parallel for schedule(static) num_threads(nthreads) if (n >= 65536)
    for (long i = 0; i < n; i++) pack_one(&hits[i], s, i);
}

/* the SoA fields a RayTraceHit needs, laid out consecutively from p for n rays */
static void hit_fields(char* p, long n, bhrt_frame_soa* s) {
    memset(s, 0, sizeof *s);
    s->result = (int32_t*)p;
    s->steps = s->result + n;
    s->hit_x = (double*)(s->steps + n);
    s->hit_y = s->hit_x + n;
    s->hit_z = s->hit_y + n;
    s->distance = s->hit_z + n;
    s->time_dilation = s->distance + n;
    s->sky_x = s->time_dilation + n;
    s->sky_y = s->sky_x + n;
    s->sky_z = s->sky_y + n;
}
#define HIT_BYTES (2 * sizeof(int32_t) + 8 * sizeof(double))

/* Large batches: K chunks per device on alternating trace streams. A device's rays are cut into
 * blocks of BHRT_BATCH_BLOCK dealt over the chunks by a repeating pattern (chunk_plan: with
 * equal weights block b goes to chunk b mod K), so every chunk carries the same mix of short
 * and long rays whatever the order of the caller's array (row-major camera rays put the
 * expensive rows in one contiguous quarter).
 * Launching chunk k first copies its blocks into consecutive pinned staging (OpenMP threads;
 * so the upload is asynchronous and overlaps the chunks already tracing); each chunk's results
 * come back in one copy on the copy stream, and the host packs a chunk into hits[] as soon as
 * it lands, with nthreads threads. BHRT_HOST_TIMING=1 prints where a call's time went. */
#define BHRT_BATCH_BLOCK 1024L

/* How a device's blocks are dealt over the K chunks: block b goes to chunk pat[b mod L], where
 * chunk k holds w[k] of the L = sum(w) pattern positions, spread evenly over the pattern (each
 * position goes to the chunk furthest behind its share), so a chunk of any weight samples the
 * whole array. Weights let the first chunk be small (the GPU starts after a short upload) and
 * the last one too (a short download and pack after the last trace); BHRT_BATCH_WEIGHTS
 * ("1,5,5,4,1") overrides the equal default. */
#define BHRT_PATTERN_MAX 64
typedef struct {
    int K, L;
    int pat[BHRT_PATTERN_MAX];
    int cnt[BHRT_MAX_CHUNKS];                   /* pattern positions of chunk k */
    int pos[BHRT_MAX_CHUNKS][BHRT_PATTERN_MAX]; /* ... in increasing order */
} chunk_plan;

static void plan_chunks(chunk_plan* P, int K, const int* w) {
    P->K = K;
    P->L = 0;
    for (int k = 0; k < K; k++) {
        P->L += w[k];
        P->cnt[k] = 0;
    }
    for (int p = 0; p < P->L; p++) {
        int best = 0;
        double lag = -1e300;
        for (int k = 0; k < K; k++) { /* share due by position p + 1 minus what k has */
            const double d = (double)w[k] * (p + 1) / P->L - P->cnt[k];
            if (d > lag + 1e-12) {
                lag = d;
                best = k;
            }
        }
        P->pat[p] = best;
        P->pos[best][P->cnt[best]++] = p;
    }
}

/* device block of chunk k's j-th block */
static inline long plan_block(const chunk_plan* P, int k, long j) {
    return (j / P->cnt[k]) * P->L + P->pos[k][j % P->cnt[k]];
}

/* rays of chunk k when a device's m rays are dealt by P (only the device's last block can be
 * partial) */
static long plan_rays(const chunk_plan* P, long m, int k) {
    const long nb = (m + BHRT_BATCH_BLOCK - 1) / BHRT_BATCH_BLOCK;
    if (nb == 0 || P->cnt[k] == 0) return 0;
    long blocks = (nb / P->L) * P->cnt[k];
    for (int t = 0; t < P->cnt[k]; t++)
        if (P->pos[k][t] < nb % P->L) blocks++;
    long rays = blocks * BHRT_BATCH_BLOCK;
    if (P->pat[(nb - 1) % P->L] == k) rays -= nb * BHRT_BATCH_BLOCK - m;
    return rays;
}

/* the chunk plan of a batch call: BHRT_BATCH_WEIGHTS; else, for >= 2^20 rays per device and
 * no BHRT_HOST_CHUNKS, weights 1,3,3,3,1 (C2's 2 M camera rays: 195-200 against 181-188
 * Mrays/s with 4 equal chunks, same box, profiles/r04/session_k_batch); else K equal chunks */
static void batch_plan(chunk_plan* P, int K, long per_dev) {
    int w[BHRT_MAX_CHUNKS], nw = 0, sum = 0;
    const char* e = getenv("BHRT_BATCH_WEIGHTS");
    if (!e && per_dev >= (1L << 20) && !getenv("BHRT_HOST_CHUNKS")) e = "1,3,3,3,1";
    while (e && *e && nw < BHRT_MAX_CHUNKS) {
        char* end;
        const long v = strtol(e, &end, 10);
        if (end == e || v < 1 || v > BHRT_PATTERN_MAX) {
            nw = 0;
            break;
        }
        w[nw++] = (int)v;
        sum += (int)v;
        e = *end == ',' ? end + 1 : end;
        if (*end != ',' && *end) {
            nw = 0;
            break;
        }
    }
    if (nw < 1 || sum > BHRT_PATTERN_MAX || (e && *e)) {
        nw = K;
        for (int k = 0; k < K; k++) w[k] = 1;
    }
    plan_chunks(P, nw, w);
}

/* chunk k of device d of a pipelined batch: its results to pinned staging on the copy stream,
 * once its trace is done (device d current) */
static int batch_download(shard_job (*jobs)[BHRT_MAX_DEV], long (*off)[BHRT_MAX_DEV], int k,
                          int d, int mk) {
    devctx_t* c = jobs[k][d].c;
    const long a = off[k][d], m = jobs[k][d].n;
    HIP_TRY(hipStreamWaitEvent(c->copy, c->chunk_done[k], 0));
    if (m > 0) /* device and staging chunks share hit_fields' layout: one copy */
        HIP_TRY(hipMemcpyAsync((char*)c->h_stage + (size_t)a * HIT_BYTES, jobs[k][d].dev.result,
                               (size_t)m * HIT_BYTES, hipMemcpyDeviceToHost, c->copy));
    HIP_TRY(hipEventRecord(c->chunk_copied[k], c->copy));
    if (mk & 8) HIP_TRY(hipEventRecord(c->tev[k][3], c->copy));
    return 0;
}

static int trace_hits_pipelined(const Ray* rays, int n, const BlackHoleParams* bh,
                                const AccretionDiskParams* dk, const SimulationConfig* cfg,
                                RayTraceHit* hits, int nthreads) {
    int ndev = bhrt_device_count();
    if (ndev <= 0) {
        set_err("no HIP device available (libbhrt has no CPU path)");
        return -1;
    }
    /* chunks per device: as for frames (frame_chunks), each chunk's copy and pack overlap the
     * next chunk's tracing; BHRT_HOST_CHUNKS overrides */
    int K = (long)n / ndev >= (1L << 20) ? 4 : 2;
    const char* env = getenv("BHRT_HOST_CHUNKS");
    if (env && atoi(env) >= 1 && atoi(env) <= BHRT_MAX_CHUNKS) K = atoi(env);
    const int stage_threads = bhrt_host_threads();
    const int timing = getenv("BHRT_HOST_TIMING") != NULL;
    const int tl = bhrt_env_int("BHRT_HOST_TIMING", 0) == 2; /* + each chunk's GPU timeline */
    /* timing events recorded (bit 0: before a chunk's upload, 1: after it, 2: after its trace,
     * 3: after its download, 4: at the call's start); BHRT_HOST_TIMING=2 records all */
    const int mk = tl ? 31 : bhrt_env_int("BHRT_BATCH_MARKERS", 0);
    /* trace streams the chunks rotate over (BHRT_BATCH_STREAMS): 2 -- with 4, every chunk
     * queued at once, C2 camera rays ran 158 instead of 172 Mrays/s (profiles/r04) */
    int nst = bhrt_env_int("BHRT_BATCH_STREAMS", 2);
    if (nst < 1) nst = 1;
    if (nst > 4) nst = 4;
    chunk_plan P;
    batch_plan(&P, K, (long)n / ndev);
    K = P.K;
    struct timespec tt[4];
    clock_gettime(CLOCK_MONOTONIC, &tt[0]);
    long d0s[BHRT_MAX_DEV], ms[BHRT_MAX_DEV];
    long off[BHRT_MAX_CHUNKS + 1][BHRT_MAX_DEV]; /* chunk k of device d: staging [off[k], off[k+1]) */
    shard_job jobs[BHRT_MAX_CHUNKS][BHRT_MAX_DEV];
    for (int d = 0; d < ndev; d++) {
        d0s[d] = (long)n * d / ndev;
        ms[d] = (long)n * (d + 1) / ndev - d0s[d];
        off[0][d] = 0;
        for (int k = 0; k < K; k++) off[k + 1][d] = off[k][d] + plan_rays(&P, ms[d], k);
        devctx_t* c = bhrt_ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (bhrt_ctx_streams(c)) return -1;
        for (int i = 0; i + 2 < nst; i++)
            if (!c->xs[i] && bhrt_own_stream(&c->xs[i])) {
                set_err("cannot create a trace stream on device %d", d);
                return -1;
            }
        const long m = ms[d];
        if (mk && !c->tev0) {
            HIP_TRY(hipEventCreate(&c->tev0));
            for (int k = 0; k < BHRT_MAX_CHUNKS; k++)
                for (int e = 0; e < 4; e++) HIP_TRY(hipEventCreate(&c->tev[k][e]));
        }
        if (mk & 16) HIP_TRY(hipEventRecord(c->tev0, c->stream));
        if (bhrt_ensure(&c->d_rays, &c->cap_rays, (size_t)m * sizeof(Ray), 0) ||
            bhrt_ensure(&c->d_soa, &c->cap_soa, (size_t)m * HIT_BYTES + 4096 * K, 0) ||
            bhrt_ensure(&c->h_rays, &c->cap_hrays, (size_t)m * sizeof(Ray), 1) ||
            bhrt_ensure(&c->h_stage, &c->cap_stage, (size_t)m * HIT_BYTES, 1))
            return -1;
    }
    for (int k = 0; k < K; k++)
        for (int d = 0; d < ndev; d++) {
            devctx_t* c = bhrt_ctx_get(d);
            const int si = k % nst;
            hipStream_t st = si == 0 ? c->stream : si == 1 ? c->stream2 : c->xs[si - 2];
            HIP_TRY(hipSetDevice(d));
            const long a = off[k][d], m = off[k + 1][d] - a, md = ms[d];
            jobs[k][d].c = c;
            jobs[k][d].n = m;
            hit_fields((char*)c->d_soa + (size_t)a * HIT_BYTES + 256 * k, m, &jobs[k][d].dev);
            if (m > 0) {
                Ray* hr = (Ray*)c->h_rays + a;
                const Ray* src = rays + d0s[d];
                const long nbk = (m + BHRT_BATCH_BLOCK - 1) / BHRT_BATCH_BLOCK;
                const Vector3D o = src[0].origin;
                /* rays that all start at src[0]'s origin travel as their directions alone
                 * (24 of 48 bytes: the upload before the chunk can start is halved); a chunk
                 * with any other origin is staged again whole */
                int diff = !bhrt_env_int("BHRT_SHARED_ORIGIN", 1);
                double* hd = (double*)hr;
                if (!diff) {
#pragma omp parallel for schedule(static) reduction(| : diff) num_threads(stage_threads) if (nbk >= 4)
                    for (long j = 0; j < nbk; j++) { /* local block j = device block plan_block() */
                        const long b0 = plan_block(&P, k, j) * BHRT_BATCH_BLOCK;
                        const long len = md - b0 < BHRT_BATCH_BLOCK ? md - b0 : BHRT_BATCH_BLOCK;
                        double* dst = hd + 3 * j * BHRT_BATCH_BLOCK;
                        for (long i = 0; i < len; i++) {
                            const Ray* r = &src[b0 + i];
                            diff |= memcmp(&r->origin, &o, sizeof o) != 0;
                            dst[3 * i] = r->direction.x;
                            dst[3 * i + 1] = r->direction.y;
                            dst[3 * i + 2] = r->direction.z;
                        }
                    }
                }
                if (diff) {
#pragma omp parallel for schedule(static) num_threads(stage_threads) if (nbk >= 4)
                    for (long j = 0; j < nbk; j++) {
                        const long b0 = plan_block(&P, k, j) * BHRT_BATCH_BLOCK;
                        const long len = md - b0 < BHRT_BATCH_BLOCK ? md - b0 : BHRT_BATCH_BLOCK;
                        memcpy(hr + j * BHRT_BATCH_BLOCK, src + b0, (size_t)len * sizeof(Ray));
                    }
                }
                const size_t bytes = (size_t)m * (diff ? sizeof(Ray) : 3 * sizeof(double));
                if (mk & 1) HIP_TRY(hipEventRecord(c->tev[k][0], st));
                HIP_TRY(hipMemcpyAsync((Ray*)c->d_rays + a, hr, bytes, hipMemcpyHostToDevice, st));
                if (mk & 2) HIP_TRY(hipEventRecord(c->tev[k][1], st));
                const Ray* dr = (const Ray*)c->d_rays + a;
                if (bhrt_rays_on_device(diff ? dr : NULL, diff ? NULL : (const double*)dr, (int)m,
                                      bh, dk, cfg, INTEGRATOR_RK4, 0, &jobs[k][d].dev, st,
                                      diff ? NULL : &o))
                    return -1;
            }
            HIP_TRY(hipEventRecord(c->chunk_done[k], st));
            if (mk & 4) HIP_TRY(hipEventRecord(c->tev[k][2], st));
            /* chunk k's download is issued after chunk k + 1's upload: both copy directions can
             * share one in-order DMA queue, and a download queued there waits for its chunk's
             * trace -- an upload issued behind it waited too, so chunk k + 1 could not start
             * before chunk k had ended and the two trace streams ran one after the other (the
             * 140 vs 205 Mrays/s "fresh-process mode" of VERDICT r5). */
            if (k > 0 && batch_download(jobs, off, k - 1, d, mk)) return -1;
            if (k == K - 1 && batch_download(jobs, off, k, d, mk)) return -1;
        }
    clock_gettime(CLOCK_MONOTONIC, &tt[1]);
    double wait_ms = 0.0, pack_ms = 0.0;
    for (int k = 0; k < K; k++)
        for (int d = 0; d < ndev; d++) {
            devctx_t* c = jobs[k][d].c;
            const long a = off[k][d], m = jobs[k][d].n;
            HIP_TRY(hipSetDevice(d));
            clock_gettime(CLOCK_MONOTONIC, &tt[2]);
            HIP_TRY(hipEventSynchronize(c->chunk_copied[k]));
            bhrt_frame_soa s;
            hit_fields((char*)c->h_stage + (size_t)a * HIT_BYTES, m, &s);
            clock_gettime(CLOCK_MONOTONIC, &tt[3]);
            RayTraceHit* h = hits + d0s[d];
            const long nbk = (m + BHRT_BATCH_BLOCK - 1) / BHRT_BATCH_BLOCK;
#pragma omp parallel for schedule(static) num_threads(nthreads) if (m >= 65536)
            for (long j = 0; j < nbk; j++) { /* local block j: rays [j B, j B + len) */
                RayTraceHit* hb = h + plan_block(&P, k, j) * BHRT_BATCH_BLOCK;
                const long i0 = j * BHRT_BATCH_BLOCK;
                const long len = m - i0 < BHRT_BATCH_BLOCK ? m - i0 : BHRT_BATCH_BLOCK;
                for (long t = 0; t < len; t++) pack_one(&hb[t], &s, i0 + t);
            }
            if (timing) {
                struct timespec t4;
                clock_gettime(CLOCK_MONOTONIC, &t4);
                wait_ms += (tt[3].tv_sec - tt[2].tv_sec) * 1e3 + (tt[3].tv_nsec - tt[2].tv_nsec) * 1e-6;
                pack_ms += (t4.tv_sec - tt[3].tv_sec) * 1e3 + (t4.tv_nsec - tt[3].tv_nsec) * 1e-6;
            }
        }
    if (timing)
        fprintf(stderr, "libbhrt trace_rays_batch n=%d K=%d: stage+issue %.2f ms, wait %.2f ms, "
                "pack %.2f ms (%d threads)\n", n, K,
                (tt[1].tv_sec - tt[0].tv_sec) * 1e3 + (tt[1].tv_nsec - tt[0].tv_nsec) * 1e-6,
                wait_ms, pack_ms, nthreads);
    if (tl) /* device 0's chunks: upload start / end, traced, downloaded (ms after the call) */
        for (int k = 0; k < K; k++) {
            devctx_t* c = jobs[k][0].c;
            float t[4] = {0, 0, 0, 0};
            for (int e = 0; e < 4; e++)
                if (jobs[k][0].n > 0 || e >= 2)
                    (void)hipEventElapsedTime(&t[e], c->tev0, c->tev[k][e]);
            fprintf(stderr, "  chunk %d (%ld rays): upload %.3f-%.3f traced %.3f downloaded %.3f\n",
                    k, jobs[k][0].n, t[0], t[1], t[2], t[3]);
        }
    return 0;
}

static int trace_into_hits(const Ray* rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           RayTraceHit* hits, int nthreads) {
    if (nthreads <= 0) nthreads = bhrt_host_threads();
    if (n >= (1 << 16)) return trace_hits_pipelined(rays, n, bh, dk, cfg, hits, nthreads);
    char* buf = (char*)malloc(HIT_BYTES * (size_t)n);
    if (!buf) {
        set_err("host allocation failed");
        return -1;
    }
    bhrt_frame_soa s;
    hit_fields(buf, n, &s);
    int rc = bhrt_trace_rays(rays, n, bh, dk, cfg, INTEGRATOR_RK4, 0, &s);
    if (rc == 0) pack_hits(hits, n, &s, 1);
    free(buf);
    return rc;
}

RayTraceResult trace_ray(const Ray* ray, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg,
                         RayTraceHit* hit) {
    if (!ray || bhrt_check_scene(bh, cfg)) return RAY_ERROR;
    RayTraceHit tmp;
    RayTraceHit* h = hit ? hit : &tmp;
    if (trace_into_hits(ray, 1, bh, dk, cfg, h, 1) != 0) {
        if (hit) hit->result = RAY_ERROR;
        return RAY_ERROR;
    }
    return h->result;
}

int trace_rays_batch(const Ray* rays, int n, const BlackHoleParams* bh,
                     const AccretionDiskParams* dk, const SimulationConfig* cfg,
                     RayTraceHit* hits, int num_threads) {
    if (!rays || !bh || !hits || n <= 0) return -1; /* raytracer.c:791-793 */
    if (!cfg) {
        set_err("config must not be NULL");
        return -1;
    }
    /* num_threads: the reference's OpenMP thread count; here the host threads that pack the
     * results into hits[] (0 = BHRT_HOST_THREADS, default 16) */
    if (trace_into_hits(rays, n, bh, dk, cfg, hits, num_threads) != 0) {
        for (int i = 0; i < n; i++) hits[i].result = RAY_ERROR;
        return -1;
    }
    return 0;
}
